// clips.hip -- recordings -> the ResNet branch's clips in ONE launch (reference: dataset.py:232-237, librosa.load(path, sr=22050)
// = channel mean + resampy 'kaiser_best', then the cut at 4 s and the zero fill). Per-output arithmetic: resample_core.h.
//
// clips_kernel: a workgroup of 256 threads owns 256 consecutive outputs of one clip (grid = clips * ceil(samples_num / 256)).
// It finds the input frames its outputs need (the positions of its first and last output, one filter wing to each side,
// clamped to [0, n_in) of ITS clip: nothing outside the clip is read), mixes them to mono while staging them in LDS with
// coalesced reads of the interleaved PCM, and every lane then runs its two wing loops on LDS: neighbouring lanes share all but
// about 1 / ratio samples. The filter taps are gathered from the clip's table (L2-resident, 512 KB, (win, delta) pairs).
// Workgroups past min(n_res, samples_num) only store zeros; a clip already at sr_out is copied (its mono mix), not filtered.
// Every element of `out` is written: no memset precedes the launch.
//
// `packed` is a buffer of BYTES: a clip has an offset into it and a sample format code (8/16/24/32-bit PCM, float32, float64;
// uniform over a workgroup), and the samples are decoded while they are staged: lanes read consecutive frames, so a wavefront's
// byte reads are contiguous. mla_clips_prepare (decoded recordings, all float32 or all int16, offsets in elements) passes one
// format for the batch and no `formats`; mla_clips_prepare_raw (the files' data chunks, offsets in bytes) passes a code per
// clip. No byte outside [offset, offset + frames * channels * bytes_per_sample) of the clip is read (resample_core.h).
#include "common.h"
#include "resample_core.h"

namespace {

using namespace resample_core;

__global__ __launch_bounds__(kThreads) void clips_kernel(const unsigned char* __restrict__ packed, const int64_t* __restrict__ offsets,
                                                         const int64_t* __restrict__ frames, const int32_t* __restrict__ channels,
                                                         const double* __restrict__ rates, const int32_t* __restrict__ table_index,
                                                         const int32_t* __restrict__ formats, int uniform_format, double sr_out,
                                                         int samples_num, int tiles, const double* __restrict__ tables, int nwin,
                                                         int num_table, int capacity, float* __restrict__ out) {
    extern __shared__ float stage[];
    const int64_t clip = blockIdx.x / tiles;
    const int t0 = int(blockIdx.x - clip * tiles) * kThreads, t = t0 + int(threadIdx.x);
    const Clip c = clip_record(clip, packed, offsets, frames, channels, rates, table_index, formats, uniform_format, tables, nwin);
    const TilePlan p = plan_tile(c, t0, sr_out, samples_num, nwin, num_table);
    float* row = out + clip * samples_num;
    if (p.mode != kFilter) {                                   // uniform over the workgroup: no barrier is skipped by part of it
        if (t < samples_num) row[t] = tile_output(c, p, t, stage, nwin, num_table);
        return;
    }
    const int count = p.count > capacity ? capacity : p.count; // never taken (span_capacity bounds it); keeps the stores inside LDS
    stage_span_raw(int(threadIdx.x), c.src, c.channels, c.format, p.first, count, stage);
    __syncthreads();
    if (t < samples_num) row[t] = tile_output(c, p, t, stage, nwin, num_table);
}

// validates one clip's rate; *floats receives the LDS floats its workgroups stage (0 for an equal rate)
int clip_lds_floats(int64_t i, double rate, double sr_out, int nwin, int num_table, int64_t* floats) {
    MLA_REQUIRE(rate > 0.0, MLA_E_ARG, "clip %lld: rate %g is not positive", (long long)i, rate);
    *floats = 0;
    if (rate == sr_out) return MLA_OK;
    const double ratio = sr_out / rate;
    const int step = index_step_of(ratio, num_table);
    MLA_REQUIRE(step >= 1, MLA_E_SHAPE, "clip %lld: ratio %g is below the filter table's resolution", (long long)i, ratio);
    MLA_REQUIRE(rate <= double(kMaxRateFactor) * sr_out, MLA_E_SHAPE, "clip %lld: rate %g is above %d x the output rate %g", (long long)i,
                rate, kMaxRateFactor, sr_out);
    *floats = span_capacity(ratio, wing_taps(nwin, step));
    return MLA_OK;
}

constexpr int64_t kMaxLdsBytes = 64 * 1024;

int lds_fits(int64_t floats) {
    MLA_REQUIRE(floats * 4 <= kMaxLdsBytes, MLA_E_SHAPE, "a workgroup would stage %lld floats, more than %lld bytes of LDS", (long long)floats,
                (long long)kMaxLdsBytes);
    return MLA_OK;
}

// Validation and launch of both entries. raw: `packed_size` and the offsets count bytes and every clip has its own format code;
// otherwise they count elements of `uniform_format` (the entry's pcm_dtype) and there are no format arrays.
int prepare(bool raw, const void* packed, int uniform_format, int64_t packed_size, int64_t clips, const int64_t* offsets, const int64_t* frames,
            const int32_t* channels, const double* rates, const int32_t* table_index, const int32_t* formats, const int64_t* host_offsets,
            const int64_t* host_frames, const int32_t* host_channels, const double* host_rates, const int32_t* host_table_index,
            const int32_t* host_formats, double sr_out, int64_t samples_num, const double* tables, int64_t n_tables, int nwin, int num_table,
            float* out, mla_stream_t stream) {
    const char* const unit = raw ? "bytes" : "elems";
    MLA_REQUIRE(clips >= 0 && samples_num >= 0 && packed_size >= 0 && n_tables >= 0, MLA_E_ARG,
                "negative size (clips %lld, samples_num %lld, packed_%s %lld, n_tables %lld)", (long long)clips, (long long)samples_num, unit,
                (long long)packed_size, (long long)n_tables);
    MLA_REQUIRE(raw || uniform_format == MLA_F32 || uniform_format == MLA_I16, MLA_E_ARG, "pcm_dtype %d is neither MLA_F32 nor MLA_I16",
                uniform_format);
    MLA_REQUIRE(sr_out > 0.0, MLA_E_ARG, "sr_out %g is not positive", sr_out);
    MLA_REQUIRE(nwin > 1 && num_table > 0, MLA_E_ARG, "bad filter table (nwin %d, num_table %d)", nwin, num_table);
    if (clips == 0) return MLA_OK;
    MLA_REQUIRE(host_offsets && host_frames && host_channels && host_rates && host_table_index && (host_formats || !raw), MLA_E_ARG,
                "null host descriptor");
    MLA_REQUIRE(offsets && frames && channels && rates && table_index && (formats || !raw), MLA_E_ARG, "null device descriptor");
    MLA_REQUIRE(out || samples_num == 0, MLA_E_ARG, "null out");
    MLA_REQUIRE(samples_num <= 0x7fffffffll - kThreads, MLA_E_SHAPE, "samples_num %lld is too large", (long long)samples_num);
    MLA_REQUIRE(!raw || reinterpret_cast<uintptr_t>(packed) % 8 == 0, MLA_E_ARG, "packed buffer %p is not aligned to 8 bytes", packed);
    int64_t most = 0;
    for (int64_t i = 0; i < clips; ++i) {
        const int64_t n = host_frames[i], off = host_offsets[i];
        const int fmt = raw ? int(host_formats[i]) : uniform_format;
        const int bytes = sample_bytes(fmt);
        MLA_REQUIRE(bytes > 0, MLA_E_ARG, "clip %lld: format code %d is no sample format", (long long)i, fmt);
        MLA_REQUIRE(n >= 0 && host_channels[i] >= 1, MLA_E_ARG, "clip %lld: %lld frames of %d channels", (long long)i, (long long)n,
                    int(host_channels[i]));
        int64_t f;
        if (int rc = clip_lds_floats(i, host_rates[i], sr_out, nwin, num_table, &f)) return rc;
        most = f > most ? f : most;
        MLA_REQUIRE(n <= (int64_t(1) << 40) / host_channels[i], MLA_E_SHAPE, "clip %lld is too long (%lld frames)", (long long)i, (long long)n);
        const int64_t size = n * host_channels[i] * (raw ? bytes : 1);
        MLA_REQUIRE(off >= 0 && off <= packed_size && size <= packed_size - off, MLA_E_ARG,
                    "clip %lld: %s [%lld, %lld) leave the packed buffer of %lld", (long long)i, raw ? "bytes" : "elements", (long long)off,
                    (long long)(off + size), (long long)packed_size);
        MLA_REQUIRE(!raw || off % sample_align(fmt) == 0, MLA_E_ARG, "clip %lld: byte offset %lld is misaligned for samples of %d bytes",
                    (long long)i, (long long)off, bytes);
        if (f > 0) {
            MLA_REQUIRE(host_table_index[i] >= 0 && host_table_index[i] < n_tables, MLA_E_ARG, "clip %lld: table %d of %lld", (long long)i,
                        int(host_table_index[i]), (long long)n_tables);
            MLA_REQUIRE(resampled_length(n, sr_out / host_rates[i]) >= 1, MLA_E_SHORT,
                        "clip %lld: input of %lld samples is too short to resample from %g to %g Hz", (long long)i, (long long)n, host_rates[i], sr_out);
        }
    }
    if (int rc = lds_fits(most)) return rc;
    if (samples_num == 0) return MLA_OK;
    MLA_REQUIRE(packed || packed_size == 0, MLA_E_ARG, "null packed buffer");
    MLA_REQUIRE(tables || most == 0, MLA_E_ARG, "null filter tables");
    const int64_t tiles = (samples_num + kThreads - 1) / kThreads;
    MLA_REQUIRE(clips * tiles <= 0x7fffffffll, MLA_E_SHAPE, "clips grid of %lld workgroups is too large", (long long)(clips * tiles));
    hipLaunchKernelGGL(clips_kernel, dim3{unsigned(clips * tiles)}, dim3{unsigned(kThreads)}, size_t(most) * sizeof(float),
                       static_cast<hipStream_t>(stream), static_cast<const unsigned char*>(packed), offsets, frames, channels, rates, table_index,
                       raw ? formats : nullptr, uniform_format, sr_out, int(samples_num), int(tiles), tables, nwin, num_table, int(most), out);
    MLA_LAUNCH_OK("clips_kernel");
    return MLA_OK;
}

}  // namespace

extern "C" int64_t mla_clips_lds_bytes(const double* host_rates, int64_t clips, double sr_out, int nwin, int num_table) {
    MLA_REQUIRE(clips >= 0 && sr_out > 0.0 && nwin > 1 && num_table > 0, MLA_E_ARG, "bad clips arguments (clips %lld, sr_out %g, nwin %d, num_table %d)",
                (long long)clips, sr_out, nwin, num_table);
    MLA_REQUIRE(host_rates || clips == 0, MLA_E_ARG, "null host_rates");
    int64_t most = 0;
    for (int64_t i = 0; i < clips; ++i) {
        int64_t f;
        if (int rc = clip_lds_floats(i, host_rates[i], sr_out, nwin, num_table, &f)) return rc;
        most = f > most ? f : most;
    }
    if (int rc = lds_fits(most)) return rc;
    return most * int64_t(sizeof(float));
}

extern "C" int mla_clips_prepare(const void* packed, int pcm_dtype, int64_t packed_elems, int64_t clips, const int64_t* offsets,
                                 const int64_t* frames, const int32_t* channels, const double* rates, const int32_t* table_index,
                                 const int64_t* host_offsets, const int64_t* host_frames, const int32_t* host_channels,
                                 const double* host_rates, const int32_t* host_table_index, double sr_out, int64_t samples_num,
                                 const double* tables, int64_t n_tables, int nwin, int num_table, float* out, mla_stream_t stream) {
    return prepare(false, packed, pcm_dtype, packed_elems, clips, offsets, frames, channels, rates, table_index, nullptr, host_offsets, host_frames,
                   host_channels, host_rates, host_table_index, nullptr, sr_out, samples_num, tables, n_tables, nwin, num_table, out, stream);
}

extern "C" int mla_clips_prepare_raw(const void* packed, int64_t packed_bytes, int64_t clips, const int64_t* offsets, const int64_t* frames,
                                     const int32_t* channels, const double* rates, const int32_t* table_index, const int32_t* formats,
                                     const int64_t* host_offsets, const int64_t* host_frames, const int32_t* host_channels,
                                     const double* host_rates, const int32_t* host_table_index, const int32_t* host_formats, double sr_out,
                                     int64_t samples_num, const double* tables, int64_t n_tables, int nwin, int num_table, float* out,
                                     mla_stream_t stream) {
    return prepare(true, packed, 0, packed_bytes, clips, offsets, frames, channels, rates, table_index, formats, host_offsets, host_frames,
                   host_channels, host_rates, host_table_index, host_formats, sr_out, samples_num, tables, n_tables, nwin, num_table, out, stream);
}
