// melspec.hip -- the ResNet branch's audio front-end on gfx950: batched power mel-dB spectrograms and the
// top_db clip + split into images (reference: dataset.py:309-316 librosa.feature.melspectrogram + power_to_db,
// dataset.py:329-363 split). Per-thread arithmetic: melspec_core.h; tables: melspec_tables.h.
//
// melspec_db_kernel: one workgroup of 256 threads owns a run of up to 16 consecutive frames of one clip. It stages
// the run's 2048 + (F - 1) * hop padded samples once in LDS (reflect indexing applied while staging; every read
// stays inside the clip's row), then per frame: windowed radix-4 FFT of 1024 complex points in LDS (5 barriers),
// even/odd split to 1025 powers, sparse mel sums (one thread per band, ascending bins, no atomics) and
// 10 log10(max(amin, .)) into a (band, frame) LDS tile. The tile is flushed band-major: the 16 frames of a band are
// consecutive in D, so every band's store is one 64-byte run. The run's maximum goes to the clip's workspace slot.
// A clip's result depends on nothing but its own samples: runs are cut per clip, never across the batch.
//
// melspec_images_kernel: reduces the clip's partial maxima (max is exact in any order and keeps NaN: a NaN sample makes its whole clip NaN, as np.maximum and .max() do), then a pure select + gather:
// out[c][t][0][band][x] = max(D[c][band][t * stride + x], Dmax_c - top_db), written as float32 or as bfloat16 (one rounding).
//
// melspec_track_db_kernel / melspec_track_max_kernel / melspec_track_images_kernel: the same spectrogram for a RAGGED batch of
// recordings of any length (no counterpart in the reference, whose loader stops at 4 s): every recording's track computed once,
// its maximum reduced once, and the distinct images of its windows gathered range by range. Index arithmetic: melspec_track_core.h.
//
// melspec_nopad_db_kernel: the same spectrogram of UNPADDED frames (center=False; the VGGish branch's librosa path,
// dataset.py:305-307, :316, with the HTK basis of mla_melspec_build_band_tables). A workgroup still owns a run of
// consecutive frames of one clip and stages its samples once, but each of its four waves owns a whole frame: its own FFT
// buffer, 4 butterflies per lane and stage, the powers written over the FFT in place, one lane per band in the mel sum
// (weights in LDS). Lanes of a wave exchange data through LDS behind wave-level fences only; the workgroup meets at three
// barriers per run (after staging, before the tile flush, in the maximum), all outside the frame loop. Per-lane arithmetic:
// melspec_wave_core.h. Nothing outside a row's first n samples is read.
#include <hip/hip_bf16.h>

#include "common.h"
#include "melspec_args.h"
#include "melspec_core.h"
#include "melspec_tables.h"
#include "melspec_track_core.h"
#include "melspec_wave_core.h"

namespace {

using namespace melspec;

// One run of a signal, the whole workgroup: frames f0 .. f0 + nf - 1 of `row`, centre-padded by reflection at its n samples, into
// out[band * frames + f0 + f] (out = the signal's (n_mels, frames) block of D). Returns the run's maximum (valid in thread 0). The
// body of melspec_db_kernel and melspec_track_db_kernel: what differs between them is only which (row, n, frames, out) a workgroup
// gets, so a column of a track and the same frame of a crop whose samples agree are the same instructions on the same values.
__device__ __forceinline__ float db_run(float* lds, int t, const float* __restrict__ row, int n, int hop, int frames, int f0, int nf,
                                        const float* __restrict__ tab, int n_mels, float amin, float* __restrict__ out) {
    float* win = lds + kLdsWin;
    float* tw = lds + kLdsTw;
    float* stage = lds + kLdsStage;
    float* zr = lds + kLdsZr;
    float* zi = lds + kLdsZi;
    float* pw = lds + kLdsPw;
    float* tile = lds + kLdsTile;
    const int* meta = reinterpret_cast<const int*>(tab + kTabMeta);
    const float* weights = tab + tab_weights(n_mels);

    for (int i = t; i < kFft + 2 * kTw; i += kThreads) lds[i] = tab[i];      // window and twiddles are contiguous in both
    stage_samples(t, row, n, f0 * hop, kFft + (nf - 1) * hop, stage);
    __syncthreads();
    float best = -INFINITY;
    for (int f = 0; f < nf; ++f) {
        fft_first(t, stage + f * hop, win, zr, zi);
        __syncthreads();
        for (int s = 1; s <= 4; ++s) {
            fft_stage(t, s, tw, zr, zi);
            __syncthreads();
        }
        power(t, tw, zr, zi, pw);
        __syncthreads();                                                   // zr / zi are free again after this barrier
        best = mla::nan_max(best, mel_db(t, pw, meta, weights, n_mels, amin, f, tile));
        // pw is next written after the following frame's five FFT barriers
    }
    __syncthreads();
    out += f0;
    for (int i = t; i < n_mels * kRunFrames; i += kThreads) {
        const int b = i / kRunFrames, f = i % kRunFrames;
        if (f < nf) out[int64_t(b) * frames + f] = tile[i];
    }
    zr[t] = best;                                                          // block maximum: zr is dead here
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) zr[t] = mla::nan_max(zr[t], zr[t + s]);
        __syncthreads();
    }
    return zr[0];
}

__global__ __launch_bounds__(kThreads) void melspec_db_kernel(const float* __restrict__ pcm, int64_t row_stride, int n, int hop,
                                                              int frames, int runs, int per_run, const float* __restrict__ tab,
                                                              int n_mels, float amin, float* __restrict__ D,
                                                              float* __restrict__ partial) {
    extern __shared__ float lds[];
    const int t = threadIdx.x;
    const int64_t clip = blockIdx.x / runs;
    const int run = int(blockIdx.x - clip * runs);
    const int f0 = run * per_run;
    const int nf = frames - f0 < per_run ? frames - f0 : per_run;
    const float best = db_run(lds, t, pcm + clip * row_stride, n, hop, frames, f0, nf, tab, n_mels, amin, D + clip * int64_t(n_mels) * frames);
    if (t == 0) partial[blockIdx.x] = best;
}

// melspec_db_kernel for a RAGGED batch (melspec_track_core.h): workgroup = one run of 16 columns of one recording's track. The runs
// of the whole batch are one item space, blockIdx.x; the recording of a run is found in the descriptors' first_run prefix (host
// built) by a binary search over scalar loads, uniform over the workgroup. The alternative, a range of workgroups per recording
// sized by the longest, would leave a batch of one long and many short recordings mostly idle. Reflection is at the track's own
// L samples, not at the row's end: nothing at or behind L is read. D_r is band-major (224, C_r) at db_offset, so a run's band
// stores stay 64-byte runs; partial[run] gets the run's maximum (nan_max: a NaN sample makes its recording's maximum NaN).
__global__ __launch_bounds__(kThreads) void melspec_track_db_kernel(const float* __restrict__ pcm, int64_t row_stride,
                                                                    const melspec_track::Rec* __restrict__ recs, int n_rec,
                                                                    const float* __restrict__ tab, float amin, float* __restrict__ D,
                                                                    float* __restrict__ partial) {
    extern __shared__ float lds[];
    const int t = threadIdx.x;
    const int rec = melspec_track::find_rec<&melspec_track::Rec::first_run>(recs, n_rec, blockIdx.x);
    const melspec_track::Rec& r = recs[rec];
    const int n = int(r.samples), frames = int(r.cols);
    const int f0 = int(blockIdx.x - r.first_run) * kRunFrames;
    const int nf = frames - f0 < kRunFrames ? frames - f0 : kRunFrames;
    const float best = db_run(lds, t, pcm + rec * row_stride, n, melspec_track::kHop, frames, f0, nf, tab, melspec_track::kMels, amin,
                              D + r.db_offset);
    if (t == 0) partial[blockIdx.x] = best;
}

// The maximum of every recording's D, reduced ONCE: one workgroup per recording over its runs' partial maxima (an hour of audio has
// about 50 000 of them; the images kernel runs once per chunk and per image and must not repeat this). Max is exact in any order.
__global__ __launch_bounds__(256) void melspec_track_max_kernel(const float* __restrict__ partial, const melspec_track::Rec* __restrict__ recs,
                                                                float* __restrict__ maxima) {
    __shared__ float red[256];
    const int t = threadIdx.x;
    const melspec_track::Rec& r = recs[blockIdx.x];
    const int64_t runs = melspec_track::runs_of(r.cols);
    float m = -INFINITY;
    for (int64_t i = t; i < runs; i += 256) m = mla::nan_max(m, partial[r.first_run + i]);
    red[t] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] = mla::nan_max(red[t], red[t + s]);
        __syncthreads();
    }
    if (t == 0) maxima[blockIdx.x] = red[0];
}

// A select and a gather: the kept images with global row in [first, first + count), out[row - first][0][band][x] =
// nan_max(D_r[band][75 u + x], max_r - top_db). 49 workgroups per image, every thread one 16-byte store of four columns (75 u is
// no multiple of 4: the loads are scalar): every element of out is written exactly once, no memset, no atomics.
__global__ __launch_bounds__(melspec_track::kImageThreads) void melspec_track_images_kernel(const float* __restrict__ D,
                                                                                          const float* __restrict__ maxima,
                                                                                          const melspec_track::Rec* __restrict__ recs,
                                                                                          int n_rec, int64_t first, float top_db,
                                                                                          float* __restrict__ out) {
    using namespace melspec_track;
    const int64_t local = blockIdx.x / kImageBlocks, row = first + local;
    const int i = int(blockIdx.x - local * kImageBlocks) * kImageThreads + threadIdx.x;
    const int band = i / (kImageW / kImageVec), x = (i % (kImageW / kImageVec)) * kImageVec;
    const int rec = find_rec<&Rec::first_image>(recs, n_rec, row);
    const Rec& r = recs[rec];
    const float lo = maxima[rec] - top_db;
    const float* src = D + db_index(r, band, image_column(row - r.first_image, r.q) + x);
    float4 v;
    v.x = mla::nan_max(src[0], lo);
    v.y = mla::nan_max(src[1], lo);
    v.z = mla::nan_max(src[2], lo);
    v.w = mla::nan_max(src[3], lo);
    *reinterpret_cast<float4*>(out + image_index(local, band, x)) = v;
}

// orders the LDS traffic of one wave's lanes among themselves: everything before it is visible to every lane after it
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kThreads) void melspec_nopad_db_kernel(const float* __restrict__ pcm, int64_t row_stride, int hop, int frames,
                                                                    int runs, int per_run, const float* __restrict__ tab, int n_mels,
                                                                    int nnz, float amin, float* __restrict__ D,
                                                                    float* __restrict__ partial) {
    extern __shared__ float lds[];
    const int t = threadIdx.x, lane = t & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(t / kWave);
    float* win = lds + kLdsWin;
    float* tw = lds + kLdsTw;
    float* stage = lds + kLdsStage;
    float* z = lds + kWLdsFft + wave * kWaveFft;
    float* wts = lds + kWLdsWeights;
    float* tile = lds + wave_lds_tile(nnz);
    const int64_t clip = blockIdx.x / runs;
    const int run = int(blockIdx.x - clip * runs);
    const int f0 = run * per_run;
    const int nf = frames - f0 < per_run ? frames - f0 : per_run;
    const int* meta = reinterpret_cast<const int*>(tab + kTabMeta);

    for (int i = t; i < kFft + 2 * kTw; i += kThreads) lds[i] = tab[i];
    for (int i = t; i < nnz; i += kThreads) wts[i] = tab[tab_weights(n_mels) + i];
    stage_plain(t, pcm + clip * row_stride, int64_t(f0) * hop, kFft + (nf - 1) * hop, stage);
    __syncthreads();
    float best = -INFINITY;
    const int rounds = (per_run + kWaves - 1) / kWaves;      // from kernel arguments only; no workgroup barrier inside the loop
    for (int r = 0; r < rounds; ++r) {
        const int f = r * kWaves + wave;
        if (f < nf) {                                        // wave-uniform: an idle frame of the clip's last run is skipped by the whole wave
            wave_fft_first(lane, stage + f * hop, win, z);
            wave_sync();
            for (int s = 1; s <= 4; ++s) {
                wave_fft_stage(lane, s, tw, z);
                wave_sync();
            }
            power_in_place(lane, tw, z);
            wave_sync();
            best = mla::nan_max(best, wave_mel_db(lane, z, meta, wts, n_mels, amin, f, tile));
            wave_sync();                                     // the next frame's first stage overwrites the powers
        }
    }
    __syncthreads();
    float* out = D + clip * int64_t(n_mels) * frames + f0;
    for (int i = t; i < n_mels * kRunFrames; i += kThreads) {
        const int b = i / kRunFrames, f = i % kRunFrames;
        if (f < nf) out[int64_t(b) * frames + f] = tile[i];
    }
    float* red = lds + kWLdsFft;                             // block maximum: the FFT buffers are dead here
    red[t] = best;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = mla::nan_max(red[t], red[t + s]);
        __syncthreads();
    }
    if (t == 0) partial[blockIdx.x] = red[0];
}

__device__ __forceinline__ void store_db(float* p, float v) { *p = v; }
__device__ __forceinline__ void store_db(__hip_bfloat16* p, float v) { *p = __float2bfloat16(v); }     // round to nearest even

template <typename OutT>
__global__ __launch_bounds__(256) void melspec_images_kernel(const float* __restrict__ D, const float* __restrict__ partial, int runs,
                                                             int n_mels, int frames, int n_images, int image_w, int stride,
                                                             float top_db, int blocks_per_clip, OutT* __restrict__ out) {
    __shared__ float red[256];
    const int t = threadIdx.x;
    const int64_t clip = blockIdx.x / blocks_per_clip;
    const int part = int(blockIdx.x - clip * blocks_per_clip);
    float m = -INFINITY;
    for (int i = t; i < runs; i += 256) m = mla::nan_max(m, partial[clip * runs + i]);
    red[t] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] = mla::nan_max(red[t], red[t + s]);
        __syncthreads();
    }
    const float lo = red[0] - top_db;
    const int64_t per_clip = int64_t(n_images) * n_mels * image_w;
    const float* src = D + clip * int64_t(n_mels) * frames;
    OutT* dst = out + clip * per_clip;
    for (int64_t i = int64_t(part) * 256 + t; i < per_clip; i += int64_t(blocks_per_clip) * 256) {
        const int x = int(i % image_w);
        const int64_t r = i / image_w;
        const int b = int(r % n_mels), img = int(r / n_mels);
        store_db(dst + i, mla::nan_max(src[int64_t(b) * frames + int64_t(img) * stride + x], lo));
    }
}

}  // namespace

extern "C" int64_t mla_melspec_frames(int64_t n_samples, int64_t hop) {
    if (n_samples < 0 || hop < 1) return -1;
    return 1 + n_samples / hop;
}

extern "C" int64_t mla_melspec_table_floats(double sr, int64_t n_mels) { return melspec::table_floats(sr, n_mels); }

extern "C" int mla_melspec_build_tables(double sr, int64_t n_mels, float* host_out) {
    MLA_REQUIRE(host_out, MLA_E_ARG, "null melspec table buffer");
    MLA_REQUIRE(melspec::valid_config(sr, n_mels), MLA_E_ARG, "melspec tables need sr > 0 and 1 <= n_mels <= %d (got sr %g, n_mels %lld)",
                kMaxMels, sr, (long long)n_mels);
    return melspec::build_tables(sr, n_mels, host_out) == 0 ? MLA_OK : ::mla::fail(MLA_E_ARG, "melspec tables could not be built");
}

extern "C" int64_t mla_melspec_workspace_bytes(int64_t clips, int64_t n_samples, int64_t hop) {
    if (clips < 0 || n_samples < 0 || hop < 1) return -1;
    return clips * runs_of(n_samples, hop) * int64_t(sizeof(float));
}

extern "C" int mla_melspec_db(const float* pcm, int64_t clips, int64_t n_samples, int64_t clip_stride, int64_t hop, int64_t n_mels,
                              float amin, const float* tables, float* out_db, float* workspace, mla_stream_t stream) {
    MLA_REQUIRE(clips >= 0, MLA_E_ARG, "melspec clips %lld < 0", (long long)clips);
    if (int rc = check_signal(n_samples, hop, n_mels)) return rc;
    MLA_REQUIRE(clip_stride >= n_samples, MLA_E_ARG, "melspec clip stride %lld < n_samples %lld", (long long)clip_stride, (long long)n_samples);
    MLA_REQUIRE(amin > 0.f, MLA_E_ARG, "melspec amin must be positive (got %g)", double(amin));
    if (clips == 0) return MLA_OK;
    MLA_REQUIRE(pcm && tables && out_db && workspace, MLA_E_ARG, "null melspec argument");
    const int64_t frames = 1 + n_samples / hop, per = run_frames(hop), runs = runs_of(n_samples, hop);
    MLA_REQUIRE(clips * runs <= 0x7fffffffll, MLA_E_SHAPE, "melspec grid of %lld workgroups is too large", (long long)(clips * runs));
    const size_t lds = size_t(lds_floats(int(n_mels))) * sizeof(float);
    MLA_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(melspec_db_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    hipLaunchKernelGGL(melspec_db_kernel, dim3(unsigned(clips * runs)), dim3(kThreads), lds, static_cast<hipStream_t>(stream), pcm,
                       clip_stride, int(n_samples), int(hop), int(frames), int(runs), int(per), tables, int(n_mels), amin, out_db, workspace);
    MLA_LAUNCH_OK("melspec_db_kernel");
    return MLA_OK;
}

namespace {
template <typename OutT>
int launch_images(const float* db, const float* workspace, int64_t clips, int64_t frames, int64_t runs, int64_t n_mels, float top_db,
                  int64_t n_images, int64_t image_w, int64_t image_stride, OutT* out, mla_stream_t stream) {
    const int64_t per_clip = n_images * n_mels * image_w;
    int64_t bpc = (per_clip + 2047) / 2048;
    bpc = bpc < 1 ? 1 : bpc > 1024 ? 1024 : bpc;
    MLA_REQUIRE(clips * bpc <= 0x7fffffffll && n_images <= 0x7fffffffll, MLA_E_SHAPE, "melspec image grid is too large");
    hipLaunchKernelGGL(melspec_images_kernel<OutT>, dim3(unsigned(clips * bpc)), dim3(256), 0, static_cast<hipStream_t>(stream), db, workspace,
                       int(runs), int(n_mels), int(frames), int(n_images), int(image_w), int(image_stride), top_db, int(bpc), out);
    MLA_LAUNCH_OK("melspec_images_kernel");
    return MLA_OK;
}
}  // namespace

extern "C" int mla_melspec_images(const float* db, const float* workspace, int64_t clips, int64_t n_samples, int64_t hop, int64_t n_mels,
                                  float top_db, int64_t n_images, int64_t image_w, int64_t image_stride, float* out, mla_stream_t stream) {
    MLA_REQUIRE(clips >= 0, MLA_E_ARG, "melspec clips %lld < 0", (long long)clips);
    if (int rc = check_signal(n_samples, hop, n_mels)) return rc;
    const int64_t frames = 1 + n_samples / hop, runs = runs_of(n_samples, hop);
    if (int rc = check_images(frames, top_db, n_images, image_w, image_stride)) return rc;
    if (clips == 0) return MLA_OK;
    MLA_REQUIRE(db && workspace && out, MLA_E_ARG, "null melspec argument");
    return launch_images(db, workspace, clips, frames, runs, n_mels, top_db, n_images, image_w, image_stride, out, stream);
}

// ---- the ResNet branch over time: ragged tracks, their maxima and the kept images (melspec_track_core.h) ----

extern "C" int mla_melspec_track_counts(int64_t n_samples, int64_t hop_images, int64_t* windows, int64_t* images, int64_t* samples,
                                        int64_t* columns) {
    MLA_REQUIRE(n_samples >= 0, MLA_E_ARG, "n_samples %lld < 0", (long long)n_samples);
    MLA_REQUIRE(hop_images >= 1 && hop_images <= melspec_track::kMaxHop, MLA_E_ARG, "hop_images %lld is not in 1 .. %lld", (long long)hop_images,
                (long long)melspec_track::kMaxHop);
    int64_t W = 0, S = 0, L = 0, C = 0;
    melspec_track::counts(n_samples, hop_images, &W, &S, &L, &C);
    if (windows) *windows = W;
    if (images) *images = S;
    if (samples) *samples = L;
    if (columns) *columns = C;
    return MLA_OK;
}

namespace {
struct TrackTotals {
    int64_t runs, cols, images;
};
// Every descriptor of the host copy against the rows and the prefixes before it, in mla_logmel_timeline's style. A set that passes
// reads and writes inside (n_samples per row, totals.runs partial maxima, 224 totals.cols floats of D, totals.images image rows).
int check_tracks(const int64_t* host_desc, int64_t recordings, int64_t n_samples, TrackTotals* totals) {
    static_assert(sizeof(melspec_track::Rec) == melspec_track::kRecFields * sizeof(int64_t), "a descriptor is six int64");
    const melspec_track::Rec* recs = reinterpret_cast<const melspec_track::Rec*>(host_desc);
    TrackTotals at{0, 0, 0};
    for (int64_t i = 0; i < recordings; ++i) {
        const melspec_track::Rec& r = recs[i];
        const int bad = melspec_track::check_rec(r, n_samples, at.runs, at.cols, at.images);
        MLA_REQUIRE(bad != 1, MLA_E_ARG, "recording %lld: hop_images %lld is not in 1 .. %lld", (long long)i, (long long)r.q,
                    (long long)melspec_track::kMaxHop);
        MLA_REQUIRE(bad != 2 || (r.samples >= melspec_track::kWindowSamples && r.samples <= melspec_track::kMaxSamples), MLA_E_SHAPE,
                    "recording %lld: a track of %lld samples is outside %lld .. 2^30", (long long)i, (long long)r.samples,
                    (long long)melspec_track::kWindowSamples);
        MLA_REQUIRE(bad != 2 && bad != 3, MLA_E_ARG, "recording %lld: %lld samples in %lld columns at hop_images %lld are no track", (long long)i,
                    (long long)r.samples, (long long)r.cols, (long long)r.q);
        MLA_REQUIRE(bad != 4, MLA_E_SHAPE, "recording %lld: the track reads %lld samples, the rows hold %lld", (long long)i, (long long)r.samples,
                    (long long)n_samples);
        MLA_REQUIRE(bad == 0, MLA_E_ARG,
                    "recording %lld: first_run %lld / db_offset %lld / first_image %lld are not the sums before it (%lld / %lld / %lld)", (long long)i,
                    (long long)r.first_run, (long long)r.db_offset, (long long)r.first_image, (long long)at.runs,
                    (long long)(at.cols * melspec_track::kMels), (long long)at.images);
        at.runs += melspec_track::runs_of(r.cols);
        at.cols += r.cols;
        at.images += melspec_track::images_of(r.samples, r.q);
        MLA_REQUIRE(at.runs <= 0x7fffffff, MLA_E_SHAPE, "too many columns for one launch (%lld runs at recording %lld)", (long long)at.runs,
                    (long long)i);
    }
    *totals = at;
    return MLA_OK;
}
}  // namespace

extern "C" int mla_melspec_track_db(const float* pcm, int64_t recordings, int64_t n_samples, int64_t row_stride, const int64_t* desc,
                                    const int64_t* host_desc, int64_t total_columns, float amin, const float* tables, float* out_db,
                                    float* workspace, float* maxima, mla_stream_t stream) {
    MLA_REQUIRE(recordings >= 0 && n_samples >= 0 && row_stride >= n_samples && total_columns >= 0, MLA_E_ARG,
                "bad recordings %lld / stride %lld < n_samples %lld / total_columns %lld", (long long)recordings, (long long)row_stride,
                (long long)n_samples, (long long)total_columns);
    MLA_REQUIRE(amin > 0.f, MLA_E_ARG, "melspec amin must be positive (got %g)", double(amin));
    if (recordings == 0) {
        MLA_REQUIRE(total_columns == 0, MLA_E_ARG, "no recordings but %lld columns", (long long)total_columns);
        return MLA_OK;
    }
    MLA_REQUIRE(pcm && desc && host_desc && tables && out_db && workspace && maxima, MLA_E_ARG, "null melspec track argument");
    MLA_REQUIRE(mla::aligned(pcm, 4) && mla::aligned(tables, 4) && mla::aligned(out_db, 4) && mla::aligned(workspace, 4) && mla::aligned(maxima, 4) &&
                    mla::aligned(desc, 8),
                MLA_E_ARG, "float buffers must be 4-byte and desc 8-byte aligned");
    MLA_REQUIRE(recordings <= 0x7fffffff, MLA_E_SHAPE, "too many recordings for one launch (%lld)", (long long)recordings);
    TrackTotals totals;
    if (int rc = check_tracks(host_desc, recordings, n_samples, &totals)) return rc;
    MLA_REQUIRE(totals.cols == total_columns, MLA_E_ARG, "the descriptors fill %lld columns, out_db has %lld", (long long)totals.cols,
                (long long)total_columns);
    const melspec_track::Rec* recs = reinterpret_cast<const melspec_track::Rec*>(desc);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = size_t(lds_floats(melspec_track::kMels)) * sizeof(float);
    MLA_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(melspec_track_db_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    hipLaunchKernelGGL(melspec_track_db_kernel, dim3(unsigned(totals.runs)), dim3(kThreads), lds, s, pcm, row_stride, recs, int(recordings), tables,
                       amin, out_db, workspace);
    MLA_LAUNCH_OK("melspec_track_db_kernel");
    hipLaunchKernelGGL(melspec_track_max_kernel, dim3(unsigned(recordings)), dim3(256), 0, s, workspace, recs, maxima);
    MLA_LAUNCH_OK("melspec_track_max_kernel");
    return MLA_OK;
}

extern "C" int mla_melspec_track_images(const float* db, const float* maxima, int64_t recordings, const int64_t* desc, const int64_t* host_desc,
                                        int64_t total_columns, float top_db, int64_t first, int64_t count, float* out, mla_stream_t stream) {
    MLA_REQUIRE(recordings >= 0 && total_columns >= 0, MLA_E_ARG, "bad recordings %lld / total_columns %lld", (long long)recordings,
                (long long)total_columns);
    MLA_REQUIRE(top_db >= 0.f, MLA_E_ARG, "melspec top_db must be non-negative (got %g)", double(top_db));
    MLA_REQUIRE(first >= 0 && count >= 0, MLA_E_ARG, "bad image range: first %lld, count %lld", (long long)first, (long long)count);
    TrackTotals totals{0, 0, 0};
    if (recordings > 0) {
        MLA_REQUIRE(host_desc, MLA_E_ARG, "null melspec track argument");
        MLA_REQUIRE(recordings <= 0x7fffffff, MLA_E_SHAPE, "too many recordings for one launch (%lld)", (long long)recordings);
        if (int rc = check_tracks(host_desc, recordings, melspec_track::kMaxSamples, &totals)) return rc;   // the images read D, not the rows
    }
    MLA_REQUIRE(totals.cols == total_columns, MLA_E_ARG, "the descriptors fill %lld columns, db has %lld", (long long)totals.cols,
                (long long)total_columns);
    MLA_REQUIRE(first <= totals.images && count <= totals.images - first, MLA_E_SHAPE, "images %lld .. %lld leave the %lld kept images",
                (long long)first, (long long)(first + count), (long long)totals.images);
    if (count == 0) return MLA_OK;
    MLA_REQUIRE(db && maxima && desc && out, MLA_E_ARG, "null melspec track argument");
    MLA_REQUIRE(mla::aligned(db, 4) && mla::aligned(maxima, 4) && mla::aligned(desc, 8) && mla::aligned(out, 16), MLA_E_ARG,
                "db and maxima must be 4-byte, desc 8-byte and out 16-byte aligned");
    MLA_REQUIRE(count <= 0x7fffffff / melspec_track::kImageBlocks, MLA_E_SHAPE, "melspec image grid is too large (%lld images)", (long long)count);
    hipLaunchKernelGGL(melspec_track_images_kernel, dim3(unsigned(count * melspec_track::kImageBlocks)), dim3(melspec_track::kImageThreads), 0,
                       static_cast<hipStream_t>(stream), db, maxima, reinterpret_cast<const melspec_track::Rec*>(desc), int(recordings), first,
                       top_db, out);
    MLA_LAUNCH_OK("melspec_track_images_kernel");
    return MLA_OK;
}

// ---- the VGGish branch's librosa path: unpadded frames (center=False), any mel basis of mla_melspec_build_band_tables ----

extern "C" int64_t mla_melspec_band_table_floats(double sr, int64_t n_mels, double fmin, double fmax, int htk) {
    return melspec::table_floats(MelConfig{sr, n_mels, fmin, fmax, htk != 0});
}

extern "C" int mla_melspec_build_band_tables(double sr, int64_t n_mels, double fmin, double fmax, int htk, float* host_out) {
    MLA_REQUIRE(host_out, MLA_E_ARG, "null melspec table buffer");
    const MelConfig c{sr, n_mels, fmin, fmax, htk != 0};
    MLA_REQUIRE(melspec::valid_config(c), MLA_E_ARG,
                "melspec tables need sr > 0, 1 <= n_mels <= %d and 0 <= fmin < fmax <= sr / 2 (got sr %g, n_mels %lld, fmin %g, fmax %g)", kMaxMels,
                sr, (long long)n_mels, fmin, fmax);
    return melspec::build_tables(c, host_out) == 0 ? MLA_OK : ::mla::fail(MLA_E_ARG, "melspec tables could not be built");
}

extern "C" int64_t mla_melspec_nopad_frames(int64_t n_samples, int64_t hop) { return nopad_frames(n_samples, hop); }

namespace {
int check_nopad_signal(int64_t n_samples, int64_t hop, int64_t n_mels) {
    MLA_REQUIRE(hop >= 1, MLA_E_ARG, "melspec hop %lld < 1", (long long)hop);
    MLA_REQUIRE(n_mels >= 1 && n_mels <= kMaxMels, MLA_E_ARG, "melspec n_mels %lld outside [1, %d]", (long long)n_mels, kMaxMels);
    MLA_REQUIRE(n_samples >= kFft, MLA_E_SHORT, "melspec without padding needs at least %d samples per clip, one whole frame (got %lld)", kFft,
                (long long)n_samples);
    MLA_REQUIRE(n_samples <= (1 << 30), MLA_E_SHAPE, "melspec clips longer than 2^30 samples are not supported (got %lld)", (long long)n_samples);
    return MLA_OK;
}
int64_t nopad_runs_of(int64_t n_samples, int64_t hop) {
    const int64_t frames = nopad_frames(n_samples, hop), per = wave_run_frames(hop);
    return (frames + per - 1) / per;
}
}  // namespace

extern "C" int64_t mla_melspec_nopad_workspace_bytes(int64_t clips, int64_t n_samples, int64_t hop) {
    if (clips < 0 || n_samples < kFft || hop < 1) return -1;
    return clips * nopad_runs_of(n_samples, hop) * int64_t(sizeof(float));
}

extern "C" int mla_melspec_nopad_db(const float* pcm, int64_t clips, int64_t n_samples, int64_t clip_stride, int64_t hop, int64_t n_mels,
                                    float amin, const float* tables, int64_t table_floats, float* out_db, float* workspace,
                                    mla_stream_t stream) {
    MLA_REQUIRE(clips >= 0, MLA_E_ARG, "melspec clips %lld < 0", (long long)clips);
    if (int rc = check_nopad_signal(n_samples, hop, n_mels)) return rc;
    MLA_REQUIRE(clip_stride >= n_samples, MLA_E_ARG, "melspec clip stride %lld < n_samples %lld", (long long)clip_stride, (long long)n_samples);
    MLA_REQUIRE(amin > 0.f, MLA_E_ARG, "melspec amin must be positive (got %g)", double(amin));
    const int64_t nnz = table_floats - tab_weights(int(n_mels));
    MLA_REQUIRE(nnz >= 0 && nnz <= kMaxWeights, MLA_E_ARG, "melspec table_floats %lld is not a table of %lld bands (%d + up to %d weights)",
                (long long)table_floats, (long long)n_mels, tab_weights(int(n_mels)), kMaxWeights);
    if (clips == 0) return MLA_OK;
    MLA_REQUIRE(pcm && tables && out_db && workspace, MLA_E_ARG, "null melspec argument");
    const int64_t frames = nopad_frames(n_samples, hop), per = wave_run_frames(hop), runs = nopad_runs_of(n_samples, hop);
    MLA_REQUIRE(clips * runs <= 0x7fffffffll, MLA_E_SHAPE, "melspec grid of %lld workgroups is too large", (long long)(clips * runs));
    const size_t lds = size_t(wave_lds_floats(int(n_mels), int(nnz))) * sizeof(float);
    MLA_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(melspec_nopad_db_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    hipLaunchKernelGGL(melspec_nopad_db_kernel, dim3(unsigned(clips * runs)), dim3(kThreads), lds, static_cast<hipStream_t>(stream), pcm,
                       clip_stride, int(hop), int(frames), int(runs), int(per), tables, int(n_mels), int(nnz), amin, out_db, workspace);
    MLA_LAUNCH_OK("melspec_nopad_db_kernel");
    return MLA_OK;
}

extern "C" int mla_melspec_nopad_bags(const float* db, const float* workspace, int64_t clips, int64_t n_samples, int64_t hop, int64_t n_mels,
                                      float top_db, int64_t n_images, int64_t image_w, int64_t image_stride, void* out, int out_dtype,
                                      mla_stream_t stream) {
    MLA_REQUIRE(clips >= 0, MLA_E_ARG, "melspec clips %lld < 0", (long long)clips);
    if (int rc = check_nopad_signal(n_samples, hop, n_mels)) return rc;
    MLA_REQUIRE(out_dtype == MLA_F32 || out_dtype == MLA_BF16, MLA_E_DTYPE, "out_dtype %d is neither MLA_F32 nor MLA_BF16", out_dtype);
    if (int rc = check_images(nopad_frames(n_samples, hop), top_db, n_images, image_w, image_stride)) return rc;
    if (clips == 0) return MLA_OK;
    MLA_REQUIRE(db && workspace && out, MLA_E_ARG, "null melspec argument");
    const int64_t frames = nopad_frames(n_samples, hop), runs = nopad_runs_of(n_samples, hop);
    if (out_dtype == MLA_BF16)
        return launch_images(db, workspace, clips, frames, runs, n_mels, top_db, n_images, image_w, image_stride, static_cast<__hip_bfloat16*>(out), stream);
    return launch_images(db, workspace, clips, frames, runs, n_mels, top_db, n_images, image_w, image_stride, static_cast<float*>(out), stream);
}
