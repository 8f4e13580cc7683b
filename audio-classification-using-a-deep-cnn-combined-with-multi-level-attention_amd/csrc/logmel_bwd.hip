// logmel_bwd.hip -- gradient of the log-mel front-end with respect to the WAVEFORM (reference: mel_features.py:71-92 stft_magnitude,
// :220-223 mel + log, framed into examples as vggish_input.py:56-76): the adjoint of frame -> Hann -> 512-point rFFT -> |.| ->
// sparse mel -> log(. + 0.01). With mla_conv1_dgrad above it, a class score's gradient reaches the audio samples.
//
//   logmel_bwd_kernel<InT>   pcm (W, n) f32 or int16 (x / 32768) with a row stride, G (W * N, 96, 64) f32 -> d_wave (W, n) f32.
//                            One launch, no workspace. Persistent 256-lane workgroups (grid cap logmel_bwd::kMaxWg), work item =
//                            (row, 14 hop-chunks of 160 samples): each of the 16 groups of 16 lanes recomputes the spectrum of one of
//                            the 16 frames that reach the chunks, pulls G back through log / mel / |.| / the real-FFT split, runs the
//                            inverse through the forward's 256-point transform (conjugated), windows, and leaves 400 floats in LDS;
//                            then every lane sums 8-9 samples' <= 3 frames in ascending frame order and stores each sample once.
//                            The mathematics, the stages and all index arithmetic are logmel_bwd_core.h, which
//                            csrc/logmel_bwd_hostsim.cpp runs on the host.
//
// Deterministic without atomics: a sample is summed by one lane in a fixed order and stored once, the zero tail included; the
// caller zeroes nothing. A row's bits depend on the row alone (not on W, the strides or the grid). 2 of 16 frames per item are
// computed twice (12.5 %). Per example: reads 61 KB of PCM (f32, each sample once from HBM, 2.86 x through L2) and 24 KB of G, writes
// 61 KB; two 256-point transforms per frame. Measured: 1.07 ms for 5 120 examples, 4.7 x the forward's vector instructions and 6.3 x
// its LDS cycles (DESIGN.md 3.16 says where they go and what would remove them).
//
// A 16-lane group never leaves its wave and a wave's LDS instructions execute in issue order, so the hand-offs between a frame's
// stages are compiler-level fences, as in logmel.hip; the two workgroup barriers of an item stand around the gather, which reads
// all 16 groups' frames.
#include "common.h"
#include "logmel_bwd_core.h"

namespace {

namespace lb = logmel_bwd;
using namespace logmel;

constexpr int kWinFloats = 416;
constexpr int kConstFloats = kTabMelW - kTabTw256;        // what logmel::load_consts reads: the 256-point twiddles and the mel window starts
constexpr int kLdsFloats = lb::kItemFrames * lb::kGroupFloats + 16 * kMelRow + kWinFloats + lb::kBwdTabFloats + kConstFloats;
constexpr int kLdsBytes = kLdsFloats * 4;
static_assert(2 * kLdsBytes <= 160 * 1024, "two workgroups per CU");

__device__ __forceinline__ void group_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename InT>
__device__ __forceinline__ float sample_of(const InT* p, int64_t at) {
    if constexpr (sizeof(InT) == 2) return float(p[at]) * (1.0f / 32768.0f);
    else return p[at];
}

template <typename InT>
__global__ __launch_bounds__(lb::kThreads, 2) void logmel_bwd_kernel(const InT* __restrict__ pcm, int64_t stride, int64_t n_samples,
                                                                  int64_t used, int64_t ipr, int64_t n_items,
                                                                  const float* __restrict__ tab, const float* __restrict__ gbtab,
                                                                  const float* __restrict__ g, float* __restrict__ d_wave,
                                                                  int64_t d_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_mel = smem + lb::kItemFrames * lb::kGroupFloats;
    float* s_win = s_mel + 16 * kMelRow;
    float* btab = s_win + kWinFloats;                        // the backward table, LDS-resident: 80 values per lane and frame
    const int t = threadIdx.x, j = t & 15, grp = t >> 4;
    float* bufA = smem + grp * lb::kGroupFloats;
    float* bufB = bufA + lb::kBufA;
    // the lane's 36 forward constants are re-read from LDS where a stage needs them: kept in registers across the item loop they
    // push the kernel over its 256 registers (two workgroups per CU) and into scratch
    float* s_const = btab + lb::kBwdTabFloats;
    for (int i = t; i < kConstFloats; i += lb::kThreads) s_const[i] = tab[kTabTw256 + i];
    for (int i = t; i < 16 * kMelRow; i += lb::kThreads) s_mel[i] = tab[kTabMelW + i];
    for (int i = t; i < kWinFloats; i += lb::kThreads) s_win[i] = tab[kTabWindow + i];
    for (int i = t; i < lb::kBwdTabFloats; i += lb::kThreads) btab[i] = gbtab[i];
    const float* melw = s_mel + kMelRow * j;
    __syncthreads();

    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        int64_t row, c0;
        lb::item_locate(item, ipr, &row, &c0);
        const int64_t f = lb::group_frame(c0, grp);
        const bool live = lb::frame_live(f, used);
        float re[16], im[16], pr[16], pi[16], ur[16], ui[16];
        if (live) {
            float x[2 * kN1];
            _Pragma("unroll") for (int n = 0; n < kN1; ++n)
                _Pragma("unroll") for (int e = 0; e < 2; ++e) {
                    const int m = lb::lane_sample(j, n, e);
                    x[2 * n + e] = m < kWin ? sample_of(pcm, lb::pcm_index(row, stride, f, m)) : 0.f;
                }
            lb::window_lane(j, x, s_win, re, im);
            LaneConsts c;
            load_consts(c, s_const - kTabTw256, j);
            phase1_fft(c, j, re, im, bufA);
        }
        group_sync();
        if (live) phase2_read(j, bufA, re, im);
        group_sync();
        if (live) {
            phase2_fft(re, im);
            lb::store_z(j, re, im, bufA);
        }
        group_sync();
        if (live) lb::split_lane(j, btab, bufA, bufB, pr, pi);
        group_sync();
        if (live) {
            float gv[4];
            _Pragma("unroll") for (int s = 0; s < 4; ++s) gv[s] = g[lb::g_index(row, used, f, band_of(j, s))];
            LaneConsts c;
            load_consts(c, s_const - kTabTw256, j);
            lb::ratio_lane(c, j, bufB, melw, gv, bufB + 256);
        }
        group_sync();
        if (live) lb::spectrum_grad_lane(j, btab, bufB + 256, pr, pi, ur, ui, bufA);
        group_sync();
        if (live) lb::join_lane(j, btab, ur, ui, bufA, re, im);
        group_sync();
        if (live) {
            LaneConsts c;
            load_consts(c, s_const - kTabTw256, j);
            lb::phase1_fft_full(c, j, re, im, bufA);
        }
        group_sync();
        if (live) phase2_read(j, bufA, re, im);
        group_sync();
        if (live) {
            phase2_fft(re, im);
            lb::window_out_lane(j, re, im, s_win, bufA);
        }
        __syncthreads();
        // the gather: lane t owns local outputs t, t + 256, ...; a sample's frames lie in groups cl .. cl + 2
        for (int i = t; i < lb::kItemChunks * kHop; i += lb::kThreads) {
            int cl, o;
            lb::out_locate(i, &cl, &o);
            const int64_t s = (c0 + cl) * kHop + o;
            if (s >= n_samples) continue;
            float acc = 0.f;
            _Pragma("unroll") for (int d = 0; d < 3; ++d) {
                const int m = lb::term_pos(o, d);
                if (m < kWin && lb::frame_live(lb::group_frame(c0, cl + d), used)) acc += smem[(cl + d) * lb::kGroupFloats + m];
            }
            d_wave[row * d_stride + s] = acc;
        }
        __syncthreads();                                     // the next item rewrites the buffers
    }
}

template <typename InT>
int launch_logmel_bwd(const void* pcm, int64_t n_wave, int64_t n_samples, int64_t stride, const float* tab, const float* btab,
                      const float* g, float* d_wave, int64_t d_stride, hipStream_t s) {
    const int64_t ipr = lb::items_per_row(n_samples), n_items = n_wave * ipr;
    MLA_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(logmel_bwd_kernel<InT>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    hipLaunchKernelGGL(logmel_bwd_kernel<InT>, dim3(lb::grid_of(n_items)), dim3(lb::kThreads), kLdsBytes, s, static_cast<const InT*>(pcm), stride,
                       n_samples, lb::used_frames(n_samples), ipr, n_items, tab, btab, g, d_wave, d_stride);
    MLA_LAUNCH_OK("logmel_bwd_kernel");
    return MLA_OK;
}

}  // namespace

extern "C" int64_t mla_logmel_bwd_table_floats(void) { return lb::kBwdTabFloats; }

extern "C" int mla_logmel_bwd_build_tables(float* host_out) {
    MLA_REQUIRE(host_out != nullptr, MLA_E_ARG, "host_out is null");
    const int rc = lb::build_bwd_tables(host_out);
    MLA_REQUIRE(rc == 0, MLA_E_SHAPE, "a frequency bin feeds more than two adjacent mel bands (%d)", rc);
    return MLA_OK;
}

extern "C" int mla_logmel_examples_bwd(const void* pcm, int pcm_dtype, int64_t n_wave, int64_t n_samples, int64_t wave_stride,
                                       const float* tables, const float* bwd_tables, const float* d_examples, float* d_wave,
                                       int64_t d_wave_stride, mla_stream_t stream) {
    MLA_REQUIRE(n_wave >= 0 && n_samples >= 0 && wave_stride >= n_samples && d_wave_stride >= n_samples, MLA_E_ARG,
                "bad n_wave %lld / n_samples %lld / strides %lld, %lld < n_samples", (long long)n_wave, (long long)n_samples,
                (long long)wave_stride, (long long)d_wave_stride);
    int64_t frames = 0, examples = 0;
    const int rc = mla_logmel_counts(n_samples, &frames, &examples);
    if (rc != MLA_OK) return rc;
    MLA_REQUIRE(pcm_dtype == MLA_F32 || pcm_dtype == MLA_I16, MLA_E_DTYPE, "pcm_dtype %d is neither MLA_F32 nor MLA_I16", pcm_dtype);
    if (n_wave == 0 || n_samples == 0) return MLA_OK;
    MLA_REQUIRE(pcm && tables && bwd_tables && d_wave && (d_examples || examples == 0), MLA_E_ARG,
                "null pcm/tables/bwd_tables/d_examples/d_wave");
    MLA_REQUIRE(mla::aligned(pcm, pcm_dtype == MLA_F32 ? 4 : 2) && mla::aligned(tables, 4) && mla::aligned(bwd_tables, 4) &&
                    mla::aligned(d_examples, 4) && mla::aligned(d_wave, 4),
                MLA_E_ARG, "pcm is misaligned for its dtype, or a float pointer is not 4-byte aligned");
    MLA_REQUIRE(n_wave <= (int64_t(1) << 40) / lb::items_per_row(n_samples), MLA_E_SHAPE, "too many waveforms for one launch (%lld)",
                (long long)n_wave);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (pcm_dtype == MLA_I16) return launch_logmel_bwd<int16_t>(pcm, n_wave, n_samples, wave_stride, tables, bwd_tables, d_examples, d_wave, d_wave_stride, s);
    return launch_logmel_bwd<float>(pcm, n_wave, n_samples, wave_stride, tables, bwd_tables, d_examples, d_wave, d_wave_stride, s);
}
