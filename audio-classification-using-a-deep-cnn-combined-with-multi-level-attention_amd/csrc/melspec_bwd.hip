// melspec_bwd.hip -- gradient of the ResNet branch's mel-dB front-end with respect to the WAVEFORM on gfx950: the adjoint of
// melspec.hip's reflect pad -> 2048-sample frames -> periodic Hann -> 2048-point rFFT -> |.|^2 -> sparse Slaney mel ->
// 10 log10(max(amin, .)) -> max(., D_max - top_db) -> split into overlapping images. With the eval trunk's backward above it
// (resnet.trunk_input_backward) a class score's gradient reaches the audio samples. The mathematics, every stage and all index
// arithmetic are melspec_bwd_core.h, which csrc/melspec_bwd_hostsim.cpp runs on the host.
//
//   melspec_images_bwd_kernel   G (clips, images, 1, bands, width), D (clips, bands, frames) and the forward's partial maxima ->
//                               dD (clips, bands, frames). One workgroup of 1024 threads per clip: the gather of the overlapping
//                               images, the floor select, and -- through one fixed tree over the workgroup -- the sum of gD over
//                               the clipped cells, added once to the first cell that holds the clip's maximum.
//   melspec_db_bwd_kernel       pcm, dD -> one span of overlap-added, windowed frame gradients per run of <= 32 frames, in the
//                               workspace. 256 threads; per frame the forward's transform (melspec_core.h), |X|^2 and the mel sums
//                               as the forward forms them, r_b, the transposed mel step as two passes over the bands of one parity
//                               (their bins are disjoint), U = 2 dP X, the real-FFT split backwards and the same radix-4 stages.
//                               15 barriers per frame; 77 888 bytes of LDS, two workgroups per CU.
//   melspec_fold_kernel         workspace -> d_pcm (clips, n): the spans that cover a padded index in run order, then the reflect
//                               fold. One store per sample; the caller zeroes nothing.
//
// float32, deterministic, no atomics, no persistent workgroup (no grid cap). The bits of a clip's gradient depend on that clip alone.
#include "common.h"
#include "melspec_args.h"
#include "melspec_bwd_core.h"

namespace {

using namespace melspec_bwd;

__global__ __launch_bounds__(kImgThreads) void melspec_images_bwd_kernel(const float* __restrict__ G, const float* __restrict__ D,
                                                                         const float* __restrict__ partial, int fwd_runs, Images s,
                                                                         float top_db, int floor_grad, float* __restrict__ dD) {
    __shared__ float red[kImgThreads];
    __shared__ int64_t cell[kImgThreads];
    const int tid = threadIdx.x;
    const int64_t clip = blockIdx.x;
    red[tid] = max_partial(tid, partial + clip * fwd_runs, fwd_runs);
    __syncthreads();
    for (int st = kImgThreads / 2; st > 0; st >>= 1) {
        max_step(tid, st, red);
        __syncthreads();
    }
    const float m = red[0], floor = m - top_db;
    __syncthreads();
    const int64_t g_clip = clip * int64_t(s.n_images) * s.n_mels * s.image_w, d_clip = clip * int64_t(s.n_mels) * s.frames;
    const Reader g{G}, d{D};
    const Writer out{dD};
    int64_t first;
    red[tid] = images_phase1(tid, g, g_clip, d, out, d_clip, s, m, floor, &first);
    cell[tid] = first;
    __syncthreads();
    for (int st = kImgThreads / 2; st > 0; st >>= 1) {
        sum_step(tid, st, red, cell);
        __syncthreads();
    }
    images_phase2(tid, g, g_clip, d, out, d_clip, s, m, floor, floor_grad ? red[0] : 0.f, cell[0]);
}

__global__ __launch_bounds__(kThreads, 2) void melspec_db_bwd_kernel(const float* __restrict__ pcm, int64_t row_stride, Runs r,
                                                                     const float* __restrict__ tab, int n_mels, float amin,
                                                                     const float* __restrict__ dD, float* __restrict__ ws) {
    extern __shared__ float lds[];
    float* win = lds + kBLdsWin;
    float* tw = lds + kBLdsTw;
    float* stage = lds + kBLdsStage;
    float* acc = lds + kBLdsAcc;
    float* zr = lds + kBLdsZr;
    float* zi = lds + kBLdsZi;
    float* pw = lds + kBLdsPw;
    float* dp = lds + kBLdsDp;
    const int t = threadIdx.x;
    const int64_t clip = blockIdx.x / r.runs;
    const int run = int(blockIdx.x - clip * r.runs);
    const int f0 = run * r.per, nf = run_count(run, r.per, r.frames), span = span_of(nf, r.hop);
    const int* meta = reinterpret_cast<const int*>(tab + kTabMeta);
    const float* weights = tab + tab_weights(n_mels);
    const float* dd = dD + clip * int64_t(n_mels) * r.frames + f0;

    for (int i = t; i < kFft + 2 * kTw; i += kThreads) lds[i] = tab[i];      // window and twiddles are contiguous in both
    stage_row(t, Reader{pcm}, clip * row_stride, r.n, f0 * r.hop, span, stage);
    for (int i = t; i < span; i += kThreads) acc[i] = 0.f;
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
        float g[2][2];
        _Pragma("unroll") for (int parity = 0; parity < 2; ++parity)
            _Pragma("unroll") for (int j = 0; j < 2; ++j) {
                const int b = pass_band(t, j, parity);
                g[parity][j] = b < n_mels ? dd[int64_t(b) * r.frames + f] : 0.f;
            }
        fft_first(t, stage + f * r.hop, win, zr, zi);
        __syncthreads();
        for (int st = 1; st <= 4; ++st) {
            fft_stage(t, st, tw, zr, zi);
            __syncthreads();
        }
        float xr[5], xi[5];
        spectrum(t, tw, zr, zi, xr, xi, pw, dp);
        __syncthreads();
        mel_pass(t, 0, pw, meta, weights, n_mels, amin, g[0], dp);
        __syncthreads();
        mel_pass(t, 1, pw, meta, weights, n_mels, amin, g[1], dp);
        __syncthreads();
        spectrum_grad(t, xr, xi, dp, pw);                                   // V: real part in dp, imaginary part over the dead powers
        __syncthreads();
        ifft_first(t, tw, dp, pw, zr, zi);
        __syncthreads();
        for (int st = 1; st <= 4; ++st) {
            fft_stage(t, st, tw, zr, zi);
            __syncthreads();
        }
        overlap_add(t, win, zr, zi, acc + f * r.hop);
        __syncthreads();                                                   // the next frame rewrites zr / zi
    }
    float* slot = ws + (clip * r.runs + run) * int64_t(r.span);
    for (int i = t; i < span; i += kThreads) slot[i] = acc[i];
}

__global__ __launch_bounds__(kFoldThreads) void melspec_fold_kernel(const float* __restrict__ ws, Runs r, int blocks_per_clip,
                                                                    float* __restrict__ d_pcm, int64_t d_stride) {
    const int64_t clip = blockIdx.x / blocks_per_clip;
    const int s = int(blockIdx.x - clip * blocks_per_clip) * kFoldThreads + threadIdx.x;
    if (s < r.n) d_pcm[clip * d_stride + s] = fold_sample(Reader{ws}, clip * int64_t(r.runs) * r.span, r, s);
}

int64_t clamp_hop(int64_t hop) { return hop < (1 << 30) ? hop : (1 << 30); }

}  // namespace

extern "C" int64_t mla_melspec_bwd_workspace_bytes(int64_t clips, int64_t n_samples, int64_t hop, int64_t n_mels) {
    if (clips < 0 || n_samples < 0 || hop < 1 || n_mels < 1) return -1;
    hop = clamp_hop(hop);
    return clips * bwd_runs(n_samples, hop) * bwd_span(hop) * int64_t(sizeof(float));
}

extern "C" int mla_melspec_images_bwd(const float* grad_images, const float* db, const float* workspace, int64_t clips, int64_t n_samples,
                                      int64_t hop, int64_t n_mels, float top_db, int64_t n_images, int64_t image_w, int64_t image_stride,
                                      int floor_grad, float* d_db, mla_stream_t stream) {
    MLA_REQUIRE(clips >= 0, MLA_E_ARG, "melspec clips %lld < 0", (long long)clips);
    if (int rc = check_signal(n_samples, hop, n_mels)) return rc;
    const int64_t frames = 1 + n_samples / hop, runs = runs_of(n_samples, hop);
    if (int rc = check_images(frames, top_db, n_images, image_w, image_stride)) return rc;
    if (clips == 0) return MLA_OK;
    MLA_REQUIRE(grad_images && db && workspace && d_db, MLA_E_ARG, "null melspec argument");
    MLA_REQUIRE(mla::aligned(grad_images, 4) && mla::aligned(db, 4) && mla::aligned(workspace, 4) && mla::aligned(d_db, 4), MLA_E_ARG,
                "melspec float buffers must be 4-byte aligned");
    MLA_REQUIRE(clips <= 0x7fffffffll && n_images <= 0x7fffffffll && runs <= 0x7fffffffll, MLA_E_SHAPE, "melspec image grid is too large");
    const Images s{int(n_mels), int(frames), int(n_images), int(image_w), int(image_stride)};
    hipLaunchKernelGGL(melspec_images_bwd_kernel, dim3(unsigned(clips)), dim3(kImgThreads), 0, static_cast<hipStream_t>(stream), grad_images, db,
                       workspace, int(runs), s, top_db, floor_grad, d_db);
    MLA_LAUNCH_OK("melspec_images_bwd_kernel");
    return MLA_OK;
}

extern "C" int mla_melspec_db_bwd(const float* pcm, int64_t clips, int64_t n_samples, int64_t clip_stride, int64_t hop, int64_t n_mels,
                                  float amin, const float* tables, const float* d_db, float* bwd_workspace, float* d_pcm, int64_t d_stride,
                                  mla_stream_t stream) {
    MLA_REQUIRE(clips >= 0, MLA_E_ARG, "melspec clips %lld < 0", (long long)clips);
    if (int rc = check_signal(n_samples, hop, n_mels)) return rc;
    MLA_REQUIRE(clip_stride >= n_samples, MLA_E_ARG, "melspec clip stride %lld < n_samples %lld", (long long)clip_stride, (long long)n_samples);
    MLA_REQUIRE(d_stride >= n_samples, MLA_E_ARG, "melspec gradient stride %lld < n_samples %lld", (long long)d_stride, (long long)n_samples);
    MLA_REQUIRE(amin > 0.f, MLA_E_ARG, "melspec amin must be positive (got %g)", double(amin));
    if (clips == 0) return MLA_OK;
    MLA_REQUIRE(pcm && tables && d_db && bwd_workspace && d_pcm, MLA_E_ARG, "null melspec argument");
    MLA_REQUIRE(mla::aligned(pcm, 4) && mla::aligned(tables, 4) && mla::aligned(d_db, 4) && mla::aligned(bwd_workspace, 4) && mla::aligned(d_pcm, 4),
                MLA_E_ARG, "melspec float buffers must be 4-byte aligned");
    const Runs r = runs_for(n_samples, clamp_hop(hop));
    const int64_t fold_blocks = (n_samples + kFoldThreads - 1) / kFoldThreads;
    MLA_REQUIRE(clips * r.runs <= 0x7fffffffll && clips * fold_blocks <= 0x7fffffffll, MLA_E_SHAPE, "melspec grid of %lld workgroups is too large",
                (long long)(clips * (r.runs > fold_blocks ? r.runs : fold_blocks)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = size_t(kBLdsFloats) * sizeof(float);
    MLA_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(melspec_db_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    hipLaunchKernelGGL(melspec_db_bwd_kernel, dim3(unsigned(clips * r.runs)), dim3(kThreads), lds, s, pcm, clip_stride, r, tables, int(n_mels), amin,
                       d_db, bwd_workspace);
    MLA_LAUNCH_OK("melspec_db_bwd_kernel");
    hipLaunchKernelGGL(melspec_fold_kernel, dim3(unsigned(clips * fold_blocks)), dim3(kFoldThreads), 0, s, bwd_workspace, r, int(fold_blocks), d_pcm,
                       d_stride);
    MLA_LAUNCH_OK("melspec_fold_kernel");
    return MLA_OK;
}
