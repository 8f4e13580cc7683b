// logmel.hip -- fused log-mel front-end for gfx950: PCM -> 0.96 s VGGish examples in one
// kernel (reference: vggish_input.py:30-82 -> mel_features.py:192-223).
//
// Roofline: HBM by bytes (algorithmic bytes per 0.96 s example: 15 360 new samples x 4 B for f32
// PCM, 2 B for int16, + 96 x 64 x 4 B out, 2 B for bf16 = 86 016 B), but what the kernel waits on
// is its own arithmetic and LDS transposes: ~600 f32 vector instructions per frame and lane
// (~1.5 MFLOP per example) and two LDS transposes per frame. Measured (rocprofv3 counters,
// profiles/): the vector pipe and the LDS are each ~50 % busy and the chip drops its clock to
// 1.9-2.1 GHz under this mix, so the design minimises instructions, LDS cycles and cache traffic
// per frame rather than chasing occupancy:
//
//   - persistent workgroups (256 threads = 16 groups of 16 lanes, 2 per CU) walk 32-frame
//     chunks grid-stride; after the table load there is NO workgroup barrier: a 16-lane group
//     never leaves its wave, so every hand-off is a wave-level fence (compiler ordering only --
//     a wave's LDS operations execute in issue order);
//   - each group owns TWO ADJACENT STFT frames per iteration. Its lanes fetch their sample pairs
//     straight from global memory (128-byte contiguous runs per group and instruction) one
//     iteration ahead, into registers. Frame B starts 160 = 5 x 32 samples after frame A, so B's
//     tap n1 is A's tap n1 + 5 under the same window value: 18 loads serve 26 taps. The remaining
//     frame overlap is served by L2; HBM sees each sample once (rocprofv3 FETCH_SIZE);
//   - radix-16 x radix-16 FFT with one LDS transpose per frame (rows of 18 complex: 16-byte
//     aligned and conflict-free for ds_read_b128), real-FFT split in registers via DPP,
//     magnitudes transposed through the dead exchange buffer, sparse triangular mel (<= 2 bands
//     per bin, 461 non-zeros, never the dense 257 x 64 product), log -- see logmel_core.h. The
//     two frames' phases are interleaved so one frame's LDS round trip hides behind the other's
//     arithmetic, and window / split twiddles / mel weights are read once per pair;
//   - finished rows are staged in the (dead) exchange buffers and leave as 16 B-per-lane stores,
//     2 KiB contiguous per wave, directly in (example, 96, 64) layout, so the 0.96 s windowing
//     (vggish_input.py:73-76) is free.
//
// Built with -fno-slp-vectorize (build.py): packed f32 has no throughput advantage on CDNA4 and
// hipcc pays ~100 v_mov shuffles per frame to form the register pairs.
#include <hip/hip_bf16.h>

#include <type_traits>

#include "common.h"
#include "conv1_core.h"
#include "logmel_bags_core.h"
#include "logmel_core.h"
#include "logmel_tables.h"
#include "logmel_timeline_core.h"

namespace {

using namespace logmel;

// Diagnostic build only (-DMLA_LOGMEL_STAMPS=1, scripts/build_variant.py): wall-clock (s_memrealtime, 100 MHz) start / end stamp of
// every workgroup, written to a buffer nothing else reads; read back through mla_debug_logmel_stamps(). The shipped kernel executes none.
#ifndef MLA_LOGMEL_STAMPS
#define MLA_LOGMEL_STAMPS 0
#endif
#if MLA_LOGMEL_STAMPS
__device__ unsigned long long g_logmel_stamps[256][10];     // per workgroup: kernel entry, end of each of its 8 waves, loop start
#endif

constexpr int kPair = 2;                                  // STFT frames per 16-lane group and iteration (adjacent frames)
constexpr int kChunk = 16 * kPair;                        // frames per workgroup iteration: a third of an example
constexpr int kThreads = 256;
constexpr int kWgPerCu = 2;                                // persistent workgroups per CU (LDS: 2 x 78 KB; 240 VGPRs)
constexpr int kXchFloats = 2 * 16 * kXchStride;           // 576 per frame in flight
constexpr int kWinFloats = 416;
constexpr int kPwPitch = 18;                              // split-twiddle row pitch: 16 rows on distinct bank pairs
constexpr int kU = 18;                                    // sample pairs per lane for two adjacent frames: 13 + 5
constexpr int kLdsFloats = kChunk * kXchFloats + 16 * kMelRow + 16 * kPwPitch + kWinFloats;
constexpr int kLdsBytes = kLdsFloats * 4;
static_assert(kWgPerCu * kLdsBytes <= 160 * 1024, "the persistent workgroups must fit one CU's LDS");
static_assert(kExFrames % kChunk == 0, "examples must split into whole chunks");
static_assert(kHop == 160 && kN1 == 13, "the frame-pair sample sharing assumes hop = 5 * 32 samples");

// group-local synchronisation. A 16-lane group never leaves its wave, and a wave's LDS
// instructions execute in issue order, so a compiler-level fence is sufficient (WAVE);
// BLOCK keeps a full workgroup barrier and exists to cross-check WAVE on hardware.
template <bool WAVE>
__device__ __forceinline__ void group_sync() {
    if (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// value held by lane (16 - j) & 15 of the same 16-lane row: DPP row_mirror (j -> 15 - j) followed by
// row_ror:1 -- two VALU moves, no LDS round trip (verified on hardware: 0 15 14 ... 1)
__device__ __forceinline__ float from_partner(float v) {
    const int m = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true);
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(m, 0x121, 0xf, 0xf, true));
}

// U[m] = (x[32 m + 2 j], x[32 m + 2 j + 1]), m < 18, relative to the first frame of the pair: frame A uses
// U[0..12], frame B (160 samples later) U[5..17]. U[17] exists for j < 8 only (B's samples 384 .. 399).
template <typename InT> struct Samples;

template <> struct Samples<float> {
    f32x2 u[kU];
    template <bool VEC>
    __device__ __forceinline__ void fetch(const float* frame, int j) {
        const float* p = frame + 2 * j;
        _Pragma("unroll") for (int m = 0; m < kU - 1; ++m) {
            u[m] = VEC ? *reinterpret_cast<const f32x2*>(p + 32 * m) : f32x2{p[32 * m], p[32 * m + 1]};
        }
        u[kU - 1] = f32x2{0.f, 0.f};
        if (j < 8) u[kU - 1] = VEC ? *reinterpret_cast<const f32x2*>(p + 32 * (kU - 1)) : f32x2{p[32 * (kU - 1)], p[32 * (kU - 1) + 1]};
    }
    __device__ __forceinline__ f32x2 pair(int m) const { return u[m]; }
};

template <> struct Samples<int16_t> {
    uint32_t u[kU];
    template <bool VEC>
    __device__ __forceinline__ void fetch(const int16_t* frame, int j) {
        const uint16_t* p = reinterpret_cast<const uint16_t*>(frame) + 2 * j;
        _Pragma("unroll") for (int m = 0; m < kU - 1; ++m) {
            u[m] = VEC ? *reinterpret_cast<const uint32_t*>(p + 32 * m) : (p[32 * m] | (uint32_t(p[32 * m + 1]) << 16));
        }
        u[kU - 1] = 0u;
        if (j < 8) u[kU - 1] = VEC ? *reinterpret_cast<const uint32_t*>(p + 32 * (kU - 1)) : (p[32 * (kU - 1)] | (uint32_t(p[32 * (kU - 1) + 1]) << 16));
    }
    // int16 -> float in [-1, 1): x / 32768 exactly (vggish_input.py:98). The result passes through an empty asm so that the
    // arithmetic after it is compiled as it is for float samples taken from registers: without it hipcc contracts the window
    // product of THIS instantiation into the first butterflies' FMAs (24 more FMAs per frame pair than the float kernel) and int16
    // PCM does not give the bits of the same samples / 32768 as float32.
    __device__ __forceinline__ f32x2 pair(int m) const {
        constexpr float k = 1.0f / 32768.0f;
        f32x2 v = f32x2{k * float(int16_t(u[m] & 0xFFFFu)), k * float(int16_t(u[m] >> 16))};
        asm("" : "+v"(v));
        return v;
    }
};

struct ChunkMap {
    int64_t wave_stride;
    int chunks_per_wave;           // examples_per_wave * 3
    __device__ __forceinline__ void locate(int64_t c, int64_t& sample0, int64_t& row0) const {
        const int64_t w = c / chunks_per_wave, r = c - w * chunks_per_wave;
        sample0 = w * wave_stride + r * (kChunk * kHop);
        row0 = c * kChunk;
    }
};

// the lane's row of the exchange buffer: 16 complex values, 16-byte aligned
__device__ __forceinline__ void read_row(const float* p, float* re, float* im) {
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p + 4 * i);
        re[2 * i] = q.x; im[2 * i] = q.y; re[2 * i + 1] = q.z; im[2 * i + 1] = q.w;
    }
}

// phase 3 of one frame: real-FFT split, magnitudes into the (dead) exchange buffer
template <bool WAVE>
__device__ __forceinline__ void split_frame(int j, const float* re, const float* im, float* xg, const float* pw) {
    float vr[8], vi[8], pr[8], pi[8];
    phase3_view(j, re, im, vr, vi);
    _Pragma("unroll") for (int s = 0; s < 8; ++s) {
        pr[s] = from_partner(vr[s]);
        pi[s] = from_partner(vi[s]);
    }
    phase3_pairs(j, re, im, pr, pi, xg, pw);
}

// phase 4 for both frames of the pair: logmel_core.h's phase4 arithmetic (same summation order per band), each
// weight vector read once. All 36 LDS reads are issued before the first FMA (the FFT registers are dead here), so
// the LDS latency is paid once, and the eight accumulators advance in turn (no dependent FMA chains).
__device__ __forceinline__ void mel_pair(const LaneConsts& c, const float* mag_a, const float* mag_b, const float* melw,
                                         float* oa, float* ob) {
    constexpr int first[4] = {0, kSlot0, kSlot0 + kSlot1, kSlot0 + kSlot1 + kSlot2};
    constexpr int count[4] = {kSlot0 / 4, kSlot1 / 4, kSlot2 / 4, kSlot3 / 4};
    f32x4 w[kTaps / 4], a[kTaps / 4], b[kTaps / 4];
    _Pragma("unroll") for (int s = 0; s < 4; ++s) {
        _Pragma("unroll") for (int t = 0; t < count[s]; ++t) {
            w[first[s] / 4 + t] = *reinterpret_cast<const f32x4*>(melw + first[s] + 4 * t);
            a[first[s] / 4 + t] = *reinterpret_cast<const f32x4*>(mag_a + c.mel_start[s] + 4 * t);
            b[first[s] / 4 + t] = *reinterpret_cast<const f32x4*>(mag_b + c.mel_start[s] + 4 * t);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    float acc_a[4] = {0.f, 0.f, 0.f, 0.f}, acc_b[4] = {0.f, 0.f, 0.f, 0.f};
    _Pragma("unroll") for (int t = 0; t < kSlot3 / 4; ++t) {
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {
            _Pragma("unroll") for (int s = 0; s < 4; ++s) {
                if (t < count[s]) {
                    acc_a[s] += w[first[s] / 4 + t][e] * a[first[s] / 4 + t][e];
                    acc_b[s] += w[first[s] / 4 + t][e] * b[first[s] / 4 + t][e];
                }
            }
        }
    }
    _Pragma("unroll") for (int s = 0; s < 4; ++s) {
        oa[s] = __builtin_amdgcn_logf(acc_a[s] + 0.01f) * 0.69314718055994530942f;
        ob[s] = __builtin_amdgcn_logf(acc_b[s] + 0.01f) * 0.69314718055994530942f;
    }
}

// four finished values -> two dwords of bf16 (round-to-nearest-even): the one rounding of a bf16 row, wherever it goes
__device__ __forceinline__ u32x2 pack_piece(f32x4 v) {
    const __hip_bfloat16 b0 = __float2bfloat16(v.x), b1 = __float2bfloat16(v.y), b2 = __float2bfloat16(v.z), b3 = __float2bfloat16(v.w);
    auto bits = [](const __hip_bfloat16& h) { return uint32_t(*reinterpret_cast<const uint16_t*>(&h)); };
    return u32x2{bits(b0) | (bits(b1) << 16), bits(b2) | (bits(b3) << 16)};
}

template <typename OutT>
__device__ __forceinline__ void store_piece(OutT* dst, f32x4 v) {
    if constexpr (sizeof(OutT) == 4) {
        *reinterpret_cast<f32x4*>(dst) = v;
    } else {
        *reinterpret_cast<u32x2*>(dst) = pack_piece(v);
    }
}

// Where the two finished rows of a frame pair go: lane j holds bands 4 j .. 4 j + 3 of row A (va) and of row B (vb).
// RowsToGlobal: (example, 96, 64) memory, one 16-byte (f32) / 8-byte (bf16) piece per lane and row.
template <typename OutT>
struct RowsToGlobal {
    OutT* dst;                                                   // row A; row B follows it
    __device__ __forceinline__ void operator()(int j, f32x4 va, f32x4 vb) const {
        store_piece<OutT>(dst + 4 * j, va);
        store_piece<OutT>(dst + kBands + 4 * j, vb);
    }
};
// RowsToStaged: bf16 rows in conv1's staged LDS layout (conv1_core.h: pitch 68, band b at column b + 1, columns 0 and 65 zero).
// Bands 4 j .. 4 j + 3 sit at columns 4 j + 1 .. 4 j + 4: a half dword, a dword, a half dword.
struct RowsToStaged {
    uint16_t* row;                                               // row A; row B is the next staged row
    __device__ __forceinline__ void one(uint16_t* r, int j, f32x4 v) const {
        const u32x2 p = pack_piece(v);
        r[4 * j + 1] = uint16_t(p.x);
        *reinterpret_cast<uint32_t*>(r + 4 * j + 2) = (p.x >> 16) | (p.y << 16);
        r[4 * j + 4] = uint16_t(p.y >> 16);
        if (j == 0) r[0] = 0;
        if (j == 15) r[65] = 0;
    }
    __device__ __forceinline__ void operator()(int j, f32x4 va, f32x4 vb) const {
        one(row, j, va);
        one(row + conv1::kPitch, j, vb);
    }
};

// ColsToStage: the wave's 8 finished rows (= 8 columns of the clip's spectrogram) side by side in its first (dead) exchange buffer,
// stage[column][band]: 16-byte pieces on write, and lane = band reads its 8 columns back conflict-free (logmel_bags_kernel).
struct ColsToStage {
    float* cols;                                                 // column of row A; row B is the next column
    __device__ __forceinline__ void operator()(int j, f32x4 va, f32x4 vb) const {
        *reinterpret_cast<f32x4*>(cols + 4 * j) = va;
        *reinterpret_cast<f32x4*>(cols + kBands + 4 * j) = vb;
    }
};

// One frame pair of a 16-lane group: window (samples already in `smp`), prefetch of the group's next pair, both FFTs, split,
// mel, log, and the two finished rows to `sink`. Shared by every kernel of this file.
template <typename InT, bool VEC, bool WAVE, typename Sink>
__device__ __forceinline__ void pair_step(const LaneConsts& c, int j, Samples<InT>& smp, const InT* next_frame, float* xa, float* xb,
                                          const float* s_win, const float* melw, const float* pw, const Sink& sink) {
    float ra[16], ia[16], rb[16], ib[16];
    {   // window: frame B's tap n1 is sample pair U[n1 + 5] under the SAME window value as A's tap n1
        _Pragma("unroll") for (int n1 = 0; n1 < kN1; ++n1) {
            const f32x2 w = *reinterpret_cast<const f32x2*>(s_win + 32 * n1 + 2 * j);   // zeros beyond 399
            const f32x2 a = smp.pair(n1), b = smp.pair(n1 + 5);
            ra[n1] = a.x * w.x; ia[n1] = a.y * w.y;
            rb[n1] = b.x * w.x; ib[n1] = b.y * w.y;
        }
    }
    if (next_frame) smp.template fetch<VEC>(next_frame, j);       // the next pair's samples fly while this one computes
    phase1_fft(c, j, ra, ia, xa);
    group_sync<WAVE>();
    phase1_fft(c, j, rb, ib, xb);
    group_sync<WAVE>();
    // both rows and the split twiddles are requested together; A's second FFT starts when ITS eight reads are back
    read_row(xa + 2 * (j * kXchStride), ra, ia);
    read_row(xb + 2 * (j * kXchStride), rb, ib);
    float pwl[16];
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {
        const f32x2 q = *reinterpret_cast<const f32x2*>(pw + 2 * i);
        pwl[2 * i] = q.x; pwl[2 * i + 1] = q.y;
    }
    __builtin_amdgcn_sched_barrier(0);
    group_sync<WAVE>();                              // every lane has requested its rows: both buffers are dead
    phase2_fft(ra, ia);
    split_frame<WAVE>(j, ra, ia, xa, pwl);           // magnitudes of A overwrite its buffer
    phase2_fft(rb, ib);
    split_frame<WAVE>(j, rb, ib, xb, pwl);
    group_sync<WAVE>();
    float oa[4], ob[4];
    mel_pair(c, xa, xb, melw, oa, ob);
    // finished rows -> floats 256..319 of the (dead) buffers, then one 16-byte piece per lane and row:
    // a wave stores its eight rows as 2 KiB contiguous
    _Pragma("unroll") for (int s = 0; s < 4; ++s) { xa[256 + band_of(j, s)] = oa[s]; xb[256 + band_of(j, s)] = ob[s]; }
    group_sync<WAVE>();
    {
        const f32x4 va = *reinterpret_cast<const f32x4*>(xa + 256 + 4 * j);
        const f32x4 vb = *reinterpret_cast<const f32x4*>(xb + 256 + 4 * j);
        group_sync<WAVE>();             // a staged sink writes LDS that other lanes have just read
        sink(j, va, vb);
    }
    group_sync<WAVE>();                 // the buffers are rewritten by the next pair
}

constexpr int kThreadsDyn = 512;                          // the persistent kernels: one workgroup per CU
constexpr int kItemFrames = 4 * kPair;                     // frames per wave-iteration

// What every kernel of this file starts from: the LDS carve-up (two exchange buffers per 16-lane group, then the tables; the
// persistent kernels' work counter follows them, and whatever a kernel adds lies behind that), the lane's constants and its table
// rows. The constructor only stores the tables; share() ends the prologue of a persistent kernel with its one workgroup barrier.
template <int THREADS>
struct Front {
    static constexpr int kFloats = (THREADS / 16) * kPair * kXchFloats + 16 * kMelRow + 16 * kPwPitch + kWinFloats;
    LaneConsts c;
    int t, j, gl, lane, wv, lane_frame;      // thread, lane of its 16-lane group, group of its wave, lane and number of its wave
    float *xa, *xb;                          // the group's exchange buffers
    float* wave_xch;                         // the wave's first exchange buffer: the 8 of its groups follow one another
    const float *melw, *pw, *s_win;          // the lane's mel weights and split twiddles; Hann window + zero tail
    int* s_next;
    int lo, hi;

    __device__ __forceinline__ Front(float* smem, const float* __restrict__ tab) {
        float* s_mel = smem + (THREADS / 16) * kPair * kXchFloats;
        float* s_pw = s_mel + 16 * kMelRow;
        float* win = s_pw + 16 * kPwPitch;
        s_win = win;
        s_next = reinterpret_cast<int*>(win + kWinFloats);
        t = threadIdx.x; j = t & 15; gl = (t >> 4) & 3; lane = t & 63; wv = __builtin_amdgcn_readfirstlane(t >> 6);
        lane_frame = kPair * gl;                                   // this group's frame pair inside an 8-frame item
        xa = smem + (kPair * (t >> 4)) * kXchFloats;
        xb = xa + kXchFloats;
        wave_xch = smem + (kItemFrames * wv) * kXchFloats;
        load_consts(c, tab, j);
        for (int i = t; i < 16 * kMelRow; i += THREADS) s_mel[i] = tab[kTabMelW + i];
        for (int i = t; i < 16 * kPwRow; i += THREADS) s_pw[(i >> 4) * kPwPitch + (i & 15)] = tab[kTabPw + i];
        for (int i = t; i < kWinFloats; i += THREADS) win[i] = tab[kTabWindow + i];
        melw = s_mel + kMelRow * j;
        pw = s_pw + kPwPitch * j;
    }
    // this workgroup's contiguous share [lo, hi) of n units (consecutive frames: the 2.5x frame overlap stays in this XCD's L2), the
    // counter its waves pull them from, and the only workgroup barrier: tables, counter and what the kernel stored before are visible
    __device__ __forceinline__ void share(int64_t n) {
        lo = int(n * int64_t(blockIdx.x) / int64_t(gridDim.x));
        hi = int(n * (int64_t(blockIdx.x) + 1) / int64_t(gridDim.x));
        if (t == 0) *s_next = lo;
        __syncthreads();
    }
    __device__ __forceinline__ int pull() const {            // wave-uniform: one lane takes the next unit of the workgroup's share
        int v = 0;
        if (lane == 0) v = atomicAdd(s_next, 1);
        return __builtin_amdgcn_readfirstlane(v);
    }
    // pair_step of this group, from `smp` to `sink`
    template <bool VEC, bool WAVE = true, typename InT, typename Sink>
    __device__ __forceinline__ void pair(Samples<InT>& smp, const InT* next_frame, const Sink& sink) const {
        pair_step<InT, VEC, WAVE>(c, j, smp, next_frame, xa, xb, s_win, melw, pw, sink);
    }
};
static_assert(Front<kThreads>::kFloats == kLdsFloats, "static kernel: LDS");

// Static kernel (cross-check build, MLA_LOGMEL_SYNC=block): 256 threads, two workgroups per CU, chunks of 32 frames dealt
// grid-stride, a full workgroup barrier at every hand-off. The reference the wave-level fences of the kernels below are tested against.
template <typename InT, typename OutT, bool VEC>
__global__ __launch_bounds__(kThreads, kWgPerCu) void logmel_kernel(const InT* __restrict__ pcm, ChunkMap map,
                                                              int64_t n_chunks, const float* __restrict__ tab,
                                                              OutT* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Front<kThreads> f(smem, tab);
    const int g = f.t >> 4, j = f.j;
    __syncthreads();                        // tables visible

    Samples<InT> smp;
    int64_t chunk = blockIdx.x, sample0, row0;
    if (chunk < n_chunks) {
        map.locate(chunk, sample0, row0);
        smp.template fetch<VEC>(pcm + sample0 + (kPair * g) * kHop, j);
    }
    for (; chunk < n_chunks; chunk += gridDim.x) {
        map.locate(chunk, sample0, row0);
        const int64_t next = chunk + gridDim.x;
        const InT* next_frame = nullptr;
        if (next < n_chunks) {
            int64_t ns, nr;
            map.locate(next, ns, nr);
            next_frame = pcm + ns + (kPair * g) * kHop;
        }
        f.template pair<VEC, false>(smp, next_frame, RowsToGlobal<OutT>{out + (row0 + kPair * g) * kBands});
    }
}

// Dynamic kernel (shipped): ONE 512-thread workgroup per CU; work item = 8 frames = one wave-iteration (4 groups x 2 frames). A
// workgroup owns a contiguous range of items and its 8 waves PULL them from an LDS counter. Why: with equal static shares the two
// waves of a SIMD do not advance equally -- vector issue is arbitrated by age, the older wave runs ~1.5x faster, finishes its share
// early and leaves its partner alone on the SIMD for the last third of the kernel (a single wave issues at half the pair's rate):
// wall-clock stamps of the static kernel showed the first-dispatched workgroup of every CU done at 225-233 us and the second at
// 335-355 us of a 358 us launch (profiles/r02_frontend_counters.txt). No workgroup barrier after the table load, no global state.
using FrontDyn = Front<kThreadsDyn>;
constexpr int kLdsFloatsDyn = FrontDyn::kFloats + 4;       // + the work counter
constexpr int kLdsBytesDyn = kLdsFloatsDyn * 4;
static_assert(kLdsBytesDyn <= 160 * 1024 && kChunk % kItemFrames == 0, "dynamic kernel: LDS / item size");

template <typename InT, typename OutT, bool VEC>
__global__ __launch_bounds__(kThreadsDyn, 1) void logmel_dyn_kernel(const InT* __restrict__ pcm, ChunkMap map, int64_t n_items,
                                                                    const float* __restrict__ tab, OutT* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
#if MLA_LOGMEL_STAMPS
    const unsigned long long stamp_entry = __builtin_amdgcn_s_memrealtime();
#endif
    FrontDyn f(smem, tab);
    f.share(n_items);
    constexpr int kQ = kChunk / kItemFrames;                  // items per 32-frame chunk of the chunk map
    auto locate_item = [&](int item, int64_t& sample, int64_t& row) {     // wave-uniform: first sample / output row of the item
        int64_t sample0, row0;
        map.locate(item / kQ, sample0, row0);
        const int fr = (item % kQ) * kItemFrames;
        sample = sample0 + int64_t(fr) * kHop;
        row = row0 + fr;
    };
    Samples<InT> smp;
    int cur = f.pull();
    int64_t sample = 0, row = 0;
    if (cur < f.hi) {
        locate_item(cur, sample, row);
        smp.template fetch<VEC>(pcm + sample + f.lane_frame * kHop, f.j);
    }
#if MLA_LOGMEL_STAMPS
    const unsigned long long stamp0 = __builtin_amdgcn_s_memrealtime();
#endif
    while (cur < f.hi) {
        const int nxt = f.pull();
        int64_t nsample = 0, nrow = 0;
        const InT* next_frame = nullptr;
        if (nxt < f.hi) {
            locate_item(nxt, nsample, nrow);
            next_frame = pcm + nsample + f.lane_frame * kHop;
        }
        f.template pair<VEC>(smp, next_frame, RowsToGlobal<OutT>{out + (row + f.lane_frame) * kBands});
        cur = nxt;
        row = nrow;
    }
#if MLA_LOGMEL_STAMPS
    if (f.lane == 0 && blockIdx.x < 256) {
        if (f.t == 0) { g_logmel_stamps[blockIdx.x][0] = stamp_entry; g_logmel_stamps[blockIdx.x][9] = stamp0; }
        g_logmel_stamps[blockIdx.x][1 + (f.t >> 6)] = __builtin_amdgcn_s_memrealtime();
    }
#endif
}

// Ragged bags (dataset.py:318-324 create_spec's native path + :329-363 split, for a batch): rows of 16 kHz PCM holding counts[c] <= 4
// whole examples each -> out[c][t][band][x] = spec_c[band][t * stride + x], where spec_c is the clip's (64, 384) spectrogram with
// 0.0 in the slots it lacks. The dynamic kernel's schedule over 48 items per clip (logmel_bags_core.h): an item of a slot the clip
// has runs pair_step, any other only stores zeros; the branch is wave-uniform. The wave's 8 columns are staged column-major in its
// first (dead) exchange buffer, then lane = band stores its 8 consecutive x (32 B of f32, 16 B of bf16) into each of the <= 3
// windows that hold the columns. Every element of `out` is written exactly once: no memset, no atomics on global memory.
static_assert(logmel_bags::kItemCols == kItemFrames && logmel_bags::kItemCols * kBands <= kXchFloats, "one item = one wave-iteration, staged in one buffer");

template <typename OutT>
__device__ __forceinline__ void store_cols(OutT* dst, f32x4 lo, f32x4 hi) {
    if constexpr (sizeof(OutT) == 4) {
        *reinterpret_cast<f32x4*>(dst) = lo;
        *reinterpret_cast<f32x4*>(dst + 4) = hi;
    } else {
        const u32x2 a = pack_piece(lo), b = pack_piece(hi);
        *reinterpret_cast<u32x4*>(dst) = u32x4{a.x, a.y, b.x, b.y};
    }
}

// The loop of the kernels that store columns (bags, timeline): a wave pulls items, runs pair_step on those that have a spectrum,
// reads the stage back as lane = band, and stores the 8 columns -- zeros for an item without a spectrum -- wherever `map` puts them.
// A Map has a Cursor (wave-uniform: where an item lies, as far as its stores need it) and
//   first(item)                          the cursor to begin from, at or before the wave's first item;
//   frame(pcm, item, lane_frame, k)      moves k forward to `item`; the first sample of this group's pair, or null for no spectrum;
//   store(out, k, lane, v_lo, v_hi)      the lane's band of the item's 8 columns to every place that holds them.
template <typename InT, typename OutT, bool VEC, typename Map>
__device__ __forceinline__ void column_items(const FrontDyn& f, const InT* __restrict__ pcm, const Map map, OutT* __restrict__ out) {
    float* stage = f.wave_xch;                                 // 8 columns x 64 bands
    Samples<InT> smp;
    int cur = f.pull();
    if (cur >= f.hi) return;
    typename Map::Cursor k = map.first(cur);
    const InT* frame = map.frame(pcm, cur, f.lane_frame, k);
    bool fetched = false;                                      // smp holds `frame`'s samples (prefetched by the item before)
    while (cur < f.hi) {
        const int nxt = f.pull();
        typename Map::Cursor kn = k;
        const InT* next_frame = nxt < f.hi ? map.frame(pcm, nxt, f.lane_frame, kn) : nullptr;
        f32x4 v_lo = {0.f, 0.f, 0.f, 0.f}, v_hi = {0.f, 0.f, 0.f, 0.f};
        if (frame) {
            // after a zero item, or at the start, nothing has been prefetched for this one
            if (!fetched) smp.template fetch<VEC>(frame, f.j);
            f.template pair<VEC>(smp, next_frame, ColsToStage{stage + f.lane_frame * kBands});
            _Pragma("unroll") for (int x = 0; x < 4; ++x) {
                v_lo[x] = stage[x * kBands + f.lane];
                v_hi[x] = stage[(4 + x) * kBands + f.lane];
            }
            group_sync<true>();             // the stage is rewritten by the next FFT
        }
        fetched = frame && next_frame;
        map.store(out, k, f.lane, v_lo, v_hi);
        cur = nxt;
        frame = next_frame;
        k = kn;
    }
}

struct BagsMap {
    const int32_t* __restrict__ counts;
    int n_frames, stride;
    int64_t row_stride;
    struct Cursor { int clip, col; };                          // the item's clip and its first column
    __device__ __forceinline__ Cursor first(int) const { return Cursor{0, 0}; }
    template <typename InT>
    __device__ __forceinline__ const InT* frame(const InT* pcm, int item, int lane_frame, Cursor& k) const {
        int slot, fr;
        logmel_bags::item_locate(item, &k.clip, &slot, &fr);
        k.col = logmel_bags::item_column(slot, fr);
        if (slot >= counts[k.clip]) return nullptr;            // the clip lacks the item's slot
        return pcm + int64_t(k.clip) * row_stride + logmel_bags::frame_sample(slot, fr + lane_frame);
    }
    template <typename OutT>
    __device__ __forceinline__ void store(OutT* out, const Cursor& k, int lane, f32x4 v_lo, f32x4 v_hi) const {
        int t_lo, t_hi;
        logmel_bags::column_windows(k.col, n_frames, stride, &t_lo, &t_hi);
        for (int w = t_lo; w <= t_hi; ++w) store_cols<OutT>(out + logmel_bags::out_offset(k.clip, n_frames, stride, w, lane, k.col), v_lo, v_hi);
    }
};

template <typename InT, typename OutT, bool VEC>
__global__ __launch_bounds__(kThreadsDyn, 1) void logmel_bags_kernel(const InT* __restrict__ pcm, int64_t row_stride,
                                                                     const int32_t* __restrict__ counts, int n_items, int n_frames,
                                                                     int stride, const float* __restrict__ tab, OutT* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    FrontDyn f(smem, tab);
    f.share(n_items);
    column_items<InT, OutT, VEC>(f, pcm, BagsMap{counts, n_frames, stride, row_stride}, out);
}

// Timeline (logmel_timeline_core.h): ragged rows of 16 kHz PCM -> the DISTINCT slots of every recording's windows at a hop of 32 q
// columns, out[slot][band][x]. The bags kernel's schedule and store over the items of the whole batch; what is new is the map from
// an item to its recording, which is ragged here. It is the descriptors' first_item prefix, built on the host: a wave finds the
// recording of its first item by a binary search and from then on walks forward (a workgroup's share is contiguous and its waves
// pull increasing items, so the walk is usually zero or one step of scalar loads). The alternative, a range of workgroups per
// recording, would leave a batch of one long and many short recordings to the few workgroups of the long one. Everything about an
// item is wave-uniform; an item of columns without a spectrum (a short recording's missing examples) only stores zeros.
struct TimelineMap {
    const logmel_timeline::Rec* __restrict__ recs;
    int n_rec, n_items;
    int64_t row_stride;
    struct Cursor {
        int rec, end_item;                   // the recording of the item and the first item past it
        int first_item, cols, spec_cols, q;
        int64_t first_slot;
        int col;                             // first column of the item
    };
    static __device__ __forceinline__ int uni(int64_t v) { return __builtin_amdgcn_readfirstlane(int(v)); }
    __device__ __forceinline__ void enter(Cursor& k, int rec) const {      // wave-uniform: the descriptor of `rec` into the cursor
        const logmel_timeline::Rec& r = recs[rec];
        k.rec = rec;
        k.first_item = uni(r.first_item);
        k.cols = uni(r.cols);
        k.spec_cols = uni(r.spec_cols);
        k.q = uni(r.q);
        k.first_slot = (int64_t(uni(r.first_slot >> 32)) << 32) | uint32_t(uni(r.first_slot));
        k.end_item = rec + 1 < n_rec ? uni(recs[rec + 1].first_item) : n_items;
    }
    __device__ __forceinline__ Cursor first(int item) const {
        Cursor k;
        enter(k, logmel_timeline::find_rec(recs, n_rec, item));
        return k;
    }
    template <typename InT>
    __device__ __forceinline__ const InT* frame(const InT* pcm, int item, int lane_frame, Cursor& k) const {
        while (item >= k.end_item) enter(k, k.rec + 1);
        k.col = logmel_timeline::item_column(item - k.first_item, k.cols, k.q);
        if (k.col >= k.spec_cols) return nullptr;              // a short recording's missing examples
        return pcm + int64_t(k.rec) * row_stride + logmel_timeline::column_sample(k.col + lane_frame);
    }
    template <typename OutT>
    __device__ __forceinline__ void store(OutT* out, const Cursor& k, int lane, f32x4 v_lo, f32x4 v_hi) const {
        _Pragma("unroll") for (int s = 0; s < logmel_timeline::kColumnSlots; ++s) {
            int row, x;
            if (logmel_timeline::column_slot(k.col, k.cols, k.q, s, &row, &x)) {
                store_cols<OutT>(out + logmel_timeline::out_offset(k.first_slot, row, lane, x), v_lo, v_hi);
            }
        }
    }
};

template <typename InT, typename OutT, bool VEC>
__global__ __launch_bounds__(kThreadsDyn, 1) void logmel_timeline_kernel(const InT* __restrict__ pcm, int64_t row_stride,
                                                                         const logmel_timeline::Rec* __restrict__ recs, int n_rec,
                                                                         int n_items, const float* __restrict__ tab, OutT* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    FrontDyn f(smem, tab);
    f.share(n_items);
    column_items<InT, OutT, VEC>(f, pcm, TimelineMap{recs, n_rec, n_items, row_stride}, out);
}

// Fused front (bf16 inference): PCM -> conv1's pooled NHWC output in one kernel; the bf16 examples never exist in memory. The
// stand-alone pair is bound by different things -- logmel_dyn_kernel by vector issue and LDS, conv1_patch_kernel by the store
// path -- so here conv1's non-temporal stores drain while other waves run FFTs.
//
// One 512-thread workgroup per CU owns a contiguous range of WHOLE CLIPS and its 8 waves pull clips from an LDS counter. A wave
// walks its clip's 12 items (8 frames each) in order, so every hand-off stays inside the wave: no workgroup barrier after the
// table load, no wait, no spin, no recomputed halo frame. After item i the wave holds input rows <= 8 i + 7, which completes
// pooled rows 4 i - 1 .. 4 i + 2 (input rows 8 i - 3 .. 8 i + 6): the item's 8 rows land as bf16 in conv1's staged layout inside
// the wave's own (dead) exchange buffers, the 3 rows before them are carried from the previous item in two pad columns of its
// exchange buffers (which every FFT otherwise rewrites), and conv1_core.h turns four pooled rows into 4 x 4 KiB of stores. Item 0
// starts at pooled row 0 with a zero row above, item 11 adds pooled row 47 with a zero row below.
// LDS: the dynamic kernel's buffers + conv1's weight fragments (8 KiB) and bias; the output stage is exchange-buffer space too.
constexpr int kClipItems = kExFrames / kItemFrames;         // 12
constexpr int kFusedWaBytes = 8 * 64 * 16;                  // A fragments of (4 positions x 2 channel tiles) x 64 lanes
constexpr int kLdsBytesFused = kLdsBytesDyn + kFusedWaBytes + 64 * 4;
constexpr int kStagedDwords = conv1::kPitch / 2;            // dwords per staged row
static_assert(kLdsBytesDyn % 16 == 0 && kLdsBytesFused <= 160 * 1024, "fused kernel: LDS");
static_assert(12 * conv1::kPitch * 2 <= kXchFloats * 4 && conv1::kStageBytes <= 2 * kXchFloats * 4 && kItemFrames * kXchFloats >= 3 * kXchFloats,
              "staged rows in the wave's first exchange buffer, output stage in the next two");
static_assert(kThreadsDyn / 64 == 8, "one wave per (position, channel tile) builds the weight fragments");

template <typename InT, bool VEC>
__global__ __launch_bounds__(kThreadsDyn, 1) void logmel_conv1_kernel(const InT* __restrict__ pcm, int64_t wave_stride, int examples,
                                                                      int n_clips, const float* __restrict__ tab,
                                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                                      mma::bf16_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    mma::u32x4* s_wa = reinterpret_cast<mma::u32x4*>(smem + kLdsFloatsDyn);
    float* s_bias = smem + kLdsFloatsDyn + kFusedWaBytes / 4;

    FrontDyn f(smem, tab);
    const int lane = f.lane;
    // the wave's 8 exchange buffers: between two FFTs, buffer 0 holds the staged input rows and buffers 1-2 the output stage
    char* wregion = reinterpret_cast<char*>(f.wave_xch);
    uint16_t* sX = reinterpret_cast<uint16_t*>(wregion);
    uint32_t* sX32 = reinterpret_cast<uint32_t*>(wregion);
    char* stage = wregion + kXchFloats * 4;

    s_wa[f.t] = __builtin_bit_cast(mma::u32x4, conv1::weight_frag(w, f.wv >> 1, f.wv & 1, lane));
    if (f.t < 64) s_bias[f.t] = bias[f.t];
    f.share(n_clips);                       // a share of whole clips; no store is in flight yet at its barrier

    auto item_frame = [&](int clip, int item) {               // first sample of this group's pair in (clip, item)
        const int wf = clip / examples, e = clip - wf * examples;
        return pcm + int64_t(wf) * wave_stride + (int64_t(e) * kExFrames + item * kItemFrames + f.lane_frame) * kHop;
    };
    Samples<InT> smp;
    int clip = f.pull(), item = 0;
    if (clip < f.hi) smp.template fetch<VEC>(item_frame(clip, 0), f.j);
    // The 3 staged rows an item hands to the next one must survive the FFTs in between, which rewrite the exchange buffers --
    // except the two pad columns of every exchange row (phase 1 writes 16 of a row's 18 complex). The pads of exchange rows
    // 9 .. 15 also lie beyond the magnitudes and the finished row (floats 0 .. 319), so nothing touches them: 28 dwords per
    // buffer. Dword d of the 102 parks in buffer 3 + d / 28 (buffers 0 .. 2 hold the staged rows and the stage).
    uint32_t* parked = reinterpret_cast<uint32_t*>(wregion) + 3 * kXchFloats;
    auto park_slot = [](int d) { return (d / 28) * kXchFloats + 2 * kXchStride * (9 + (d % 28) / 4) + 32 + d % 4; };
    const int second = 64 + lane < 3 * kStagedDwords ? 64 + lane : 3 * kStagedDwords - 1;
    // conv1 of one finished item: staged rows 3 .. 10 are in place (written by the item's FFT pass)
    auto conv_item = [&](int clip, int item) {
        {   // rows 0 .. 2 = 102 dwords, parked by the previous item (zero at a clip's start)
            const uint32_t k0 = parked[park_slot(lane)], k1 = parked[park_slot(second)];
            sX32[lane] = item == 0 ? 0u : k0;
            if (lane < 3 * kStagedDwords - 64) sX32[64 + lane] = item == 0 ? 0u : k1;
        }
        if (lane < kStagedDwords) sX32[11 * kStagedDwords + lane] = 0u;         // row 11: the zero row below the clip (read by item 11 only)
        group_sync<true>();
        {
            mma::bf16x8 wa[4][2];
            conv1::f32x16 binit[2];
            _Pragma("unroll") for (int pos = 0; pos < 4; ++pos)
                _Pragma("unroll") for (int mt = 0; mt < 2; ++mt) wa[pos][mt] = __builtin_bit_cast(mma::bf16x8, s_wa[(pos * 2 + mt) * 64 + lane]);
            _Pragma("unroll") for (int mt = 0; mt < 2; ++mt) binit[mt] = conv1::bias_frag(s_bias, mt, lane);
            // pooled row 4 item - 1 + q from staged rows 2 q .. 2 q + 3. Item 0 has no q = 0 (pooled row -1): it writes its q = 1
            // twice, so that every item issues the same 16 stores in straight-line code. Item 11's fifth row, the clip's last,
            // goes first, under a uniform branch.
            auto row = [&](int q) {
                char* gdst = reinterpret_cast<char*>(out + ((size_t(clip) * 48 + size_t(4 * item - 1 + q)) * 32) * 64);
                conv1::pooled_row(sX + (2 * q) * conv1::kPitch, wa, binit, stage, gdst, lane);
            };
            if (item == kClipItems - 1) row(4);
            row(item == 0 ? 1 : 0);
            row(1);
            row(2);
            row(3);
        }
        {   // rows 8 .. 10 become rows 0 .. 2 of the next item
            const uint32_t k0 = sX32[8 * kStagedDwords + lane], k1 = sX32[8 * kStagedDwords + second];
            parked[park_slot(lane)] = k0;
            parked[park_slot(second)] = k1;         // lanes past the end rewrite the last dword with its own value
        }
        group_sync<true>();                 // the staged rows and the stage are rewritten by the next FFT
    };
    while (clip < f.hi) {
        int nclip = clip, nitem = item + 1;
        if (nitem == kClipItems) { nclip = f.pull(); nitem = 0; }
        const InT* next_frame = nclip < f.hi ? item_frame(nclip, nitem) : nullptr;
        // staged row r <-> input row 8 item - 3 + r: this item's rows are r = 3 .. 10
        f.template pair<VEC>(smp, next_frame, RowsToStaged{sX + (3 + f.lane_frame) * conv1::kPitch});
        conv_item(clip, item);
        clip = nclip;
        item = nitem;
    }
}

// One launch of a persistent kernel: `per_cu` workgroups on every CU, but no more than `want` (the units there are to share out).
template <typename Kern, typename... Args>
int launch_persistent(Kern kern, const char* name, int threads, int per_cu, int lds_bytes, int64_t want, hipStream_t stream, Args... args) {
    const int64_t slots = per_cu * int64_t(mla::cu_count());
    const int64_t wgs = want < slots ? want : slots;
    MLA_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    hipLaunchKernelGGL(kern, dim3(unsigned(wgs)), dim3(threads), lds_bytes, stream, args...);
    MLA_LAUNCH_OK(name);
    return MLA_OK;
}
constexpr int64_t item_wgs(int64_t n_items) { return (n_items + 7) / 8; }      // an item for each of a workgroup's 8 waves

// fn(InT{}, vec): vec is std::true_type where a lane's sample pair can be one load, which needs every row to begin at a pair
template <typename InT, typename Fn>
int by_pair_loads(const void* pcm, int64_t row_stride, Fn&& fn) {
    const bool vec = mla::aligned(pcm, 2 * sizeof(InT)) && (row_stride % 2 == 0);
    return vec ? fn(InT{}, std::true_type{}) : fn(InT{}, std::false_type{});
}
// The dtype dispatch of every entry: fn(InT{}, vec) for the fused entry, fn(InT{}, OutT{}, vec) for the others.
template <typename Fn>
int by_pcm(int pcm_dtype, const void* pcm, int64_t row_stride, Fn&& fn) {
    return pcm_dtype == MLA_F32 ? by_pair_loads<float>(pcm, row_stride, fn) : by_pair_loads<int16_t>(pcm, row_stride, fn);
}
template <typename Fn>
int by_dtypes(int pcm_dtype, int out_dtype, const void* pcm, int64_t row_stride, Fn&& fn) {
    return by_pcm(pcm_dtype, pcm, row_stride, [&](auto in, auto vec) {
        return out_dtype == MLA_F32 ? fn(in, float{}, vec) : fn(in, __hip_bfloat16{}, vec);
    });
}

// What every entry requires of its dtypes and of the pointers all of them take. Two steps, because the bags and timeline entries
// refuse an unknown dtype even for an empty batch, whose pointers may be null. `spell`: those two entries name the dtypes they take.
int check_dtypes(int pcm_dtype, int out_dtype, bool spell) {
    MLA_REQUIRE(pcm_dtype == MLA_F32 || pcm_dtype == MLA_I16, MLA_E_DTYPE, "pcm_dtype %d%s", pcm_dtype, spell ? " is neither MLA_F32 nor MLA_I16" : "");
    MLA_REQUIRE(out_dtype == MLA_F32 || out_dtype == MLA_BF16, MLA_E_DTYPE, "out_dtype %d%s", out_dtype, spell ? " is neither MLA_F32 nor MLA_BF16" : "");
    return MLA_OK;
}
int check_pointers(const void* pcm, int pcm_dtype, const float* tables, const void* out, const char* tables_text) {
    MLA_REQUIRE(mla::aligned(out, 16), MLA_E_ARG, "out must be 16-byte aligned");
    MLA_REQUIRE(mla::aligned(tables, 4), MLA_E_ARG, "%s", tables_text);
    MLA_REQUIRE(mla::aligned(pcm, pcm_dtype == MLA_F32 ? 4 : 2), MLA_E_ARG, "pcm misaligned for its dtype");
    return MLA_OK;
}

}  // namespace

#if MLA_LOGMEL_STAMPS
extern "C" int mla_debug_logmel_stamps(unsigned long long* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_logmel_stamps), sizeof(g_logmel_stamps)) == hipSuccess ? 0 : -4;
}
#endif

extern "C" int mla_logmel_counts(int64_t n_samples, int64_t* stft_frames, int64_t* examples) {
    // mel_features.py:42: 1 + int(floor((n - 400) / 160)); negative counts raise in as_strided.
    MLA_REQUIRE(n_samples >= 0, MLA_E_ARG, "n_samples %lld < 0", (long long)n_samples);
    const int64_t d = n_samples - kWin;
    const int64_t fl = d >= 0 ? d / kHop : -((-d + kHop - 1) / kHop);      // floor division
    const int64_t frames = 1 + fl;
    MLA_REQUIRE(frames >= 0, MLA_E_SHORT, "waveform of %lld samples gives a negative frame count (reference raises ValueError)",
                (long long)n_samples);
    const int64_t d2 = frames - kExFrames;
    const int64_t fl2 = d2 >= 0 ? d2 / kExFrames : -((-d2 + kExFrames - 1) / kExFrames);
    const int64_t ex = 1 + fl2;
    if (stft_frames) *stft_frames = frames;
    if (examples) *examples = ex > 0 ? ex : 0;
    return MLA_OK;
}

extern "C" int64_t mla_logmel_table_floats(void) { return kTabFloats; }

extern "C" int mla_logmel_build_tables(float* host_out) {
    MLA_REQUIRE(host_out != nullptr, MLA_E_ARG, "host_out is null");
    const int rc = build_tables(host_out);
    MLA_REQUIRE(rc == 0, MLA_E_SHAPE, "mel band structure does not fit the kernel's padded slots (%d)", rc);
    return MLA_OK;
}

extern "C" int mla_logmel_reference_tables(double* host_window400, double* host_mel_257x64) {
    MLA_REQUIRE(host_window400 && host_mel_257x64, MLA_E_ARG, "null output");
    hann400(host_window400);
    mel_dense(host_mel_257x64);
    return MLA_OK;
}

extern "C" int mla_logmel_examples(const void* pcm, int pcm_dtype, int64_t n_wave, int64_t n_samples,
                                   int64_t wave_stride, const float* tables, void* out, int out_dtype,
                                   mla_stream_t stream) {
    MLA_REQUIRE(n_wave >= 0 && wave_stride >= n_samples, MLA_E_ARG, "bad n_wave %lld / stride %lld < n_samples %lld",
                (long long)n_wave, (long long)wave_stride, (long long)n_samples);
    int64_t frames = 0, examples = 0;
    const int rc = mla_logmel_counts(n_samples, &frames, &examples);
    if (rc != MLA_OK) return rc;
    if (n_wave == 0 || examples == 0) return MLA_OK;
    MLA_REQUIRE(pcm && tables && out, MLA_E_ARG, "null pcm/tables/out");
    if (const int bad = check_dtypes(pcm_dtype, out_dtype, false); bad != MLA_OK) return bad;
    if (const int bad = check_pointers(pcm, pcm_dtype, tables, out, "out must be 16-byte aligned"); bad != MLA_OK) return bad;
    const int64_t n_chunks = n_wave * examples * (kExFrames / kChunk), n_items = n_chunks * (kChunk / kItemFrames);
    const ChunkMap map{wave_stride, int(examples * (kExFrames / kChunk))};
    // MLA_LOGMEL_SYNC=block: the cross-check build of the group sync (static kernel, full barriers)
    const char* env = getenv("MLA_LOGMEL_SYNC");
    const bool block_sync = env && env[0] == 'b';
    MLA_REQUIRE(block_sync || n_items <= 0x7fffffff, MLA_E_SHAPE, "too many frames for one launch (%lld items)", (long long)n_items);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_dtypes(pcm_dtype, out_dtype, pcm, wave_stride, [&](auto in, auto o, auto vec) {
        using InT = decltype(in);
        using OutT = decltype(o);
        constexpr bool kVec = decltype(vec)::value;
        if (block_sync) {
            return launch_persistent(logmel_kernel<InT, OutT, kVec>, "logmel_kernel", kThreads, kWgPerCu, kLdsBytes, n_chunks, s,
                                     static_cast<const InT*>(pcm), map, n_chunks, tables, static_cast<OutT*>(out));
        }
        // shipped: one 512-thread workgroup per CU, waves pull 8-frame items from an LDS counter
        return launch_persistent(logmel_dyn_kernel<InT, OutT, kVec>, "logmel_dyn_kernel", kThreadsDyn, 1, kLdsBytesDyn, item_wgs(n_items), s,
                                 static_cast<const InT*>(pcm), map, n_items, tables, static_cast<OutT*>(out));
    });
}

extern "C" int mla_logmel_bags(const void* pcm, int pcm_dtype, int64_t clips, int64_t n_samples, int64_t row_stride,
                               const int32_t* counts, const int32_t* host_counts, int n_frames, int stride, const float* tables,
                               void* out, int out_dtype, mla_stream_t stream) {
    MLA_REQUIRE(clips >= 0 && n_samples >= 0 && row_stride >= n_samples, MLA_E_ARG, "bad clips %lld / stride %lld < n_samples %lld",
                (long long)clips, (long long)row_stride, (long long)n_samples);
    if (const int bad = check_dtypes(pcm_dtype, out_dtype, true); bad != MLA_OK) return bad;
    MLA_REQUIRE(logmel_bags::config_ok(n_frames, stride), MLA_E_SHAPE,
                "%d frames at stride %d: only (10, 32) and (4, 96) are compiled (dataset.py:352-361)", n_frames, stride);
    if (clips == 0) return MLA_OK;
    MLA_REQUIRE(pcm && counts && host_counts && tables && out, MLA_E_ARG, "null pcm/counts/host_counts/tables/out");
    if (const int bad = check_pointers(pcm, pcm_dtype, tables, out, "tables and counts must be 4-byte aligned"); bad != MLA_OK) return bad;
    MLA_REQUIRE(mla::aligned(counts, 4), MLA_E_ARG, "tables and counts must be 4-byte aligned");
    MLA_REQUIRE(clips <= 0x7fffffff / logmel_bags::kClipItems, MLA_E_SHAPE, "too many clips for one launch (%lld)", (long long)clips);
    for (int64_t i = 0; i < clips; ++i) {
        const int n = host_counts[i];
        MLA_REQUIRE(n >= 0 && n <= logmel_bags::kSlots, MLA_E_ARG, "clip %lld: %d examples do not fit the 4 slots (dataset.py:321-322)",
                    (long long)i, n);
        MLA_REQUIRE(logmel_bags::samples_read(n) <= n_samples, MLA_E_SHAPE, "clip %lld: %d examples read %lld samples, the rows hold %lld",
                    (long long)i, n, (long long)logmel_bags::samples_read(n), (long long)n_samples);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n_items = clips * logmel_bags::kClipItems;
    return by_dtypes(pcm_dtype, out_dtype, pcm, row_stride, [&](auto in, auto o, auto vec) {
        using InT = decltype(in);
        using OutT = decltype(o);
        return launch_persistent(logmel_bags_kernel<InT, OutT, decltype(vec)::value>, "logmel_bags_kernel", kThreadsDyn, 1, kLdsBytesDyn,
                                 item_wgs(n_items), s, static_cast<const InT*>(pcm), row_stride, counts, int(n_items), n_frames, stride, tables,
                                 static_cast<OutT*>(out));
    });
}

extern "C" int mla_timeline_counts(int64_t n_samples, int64_t hop_slots, int64_t* windows, int64_t* slots, int64_t* samples_read) {
    MLA_REQUIRE(n_samples >= 0, MLA_E_ARG, "n_samples %lld < 0", (long long)n_samples);
    MLA_REQUIRE(hop_slots >= 1 && hop_slots <= logmel_timeline::kMaxCols, MLA_E_ARG, "hop_slots %lld is not in 1 .. %lld", (long long)hop_slots,
                (long long)logmel_timeline::kMaxCols);
    int64_t W = 0, S = 0, cols = 0, spec = 0;
    MLA_REQUIRE(logmel_timeline::counts(n_samples, hop_slots, &W, &S, &cols, &spec), MLA_E_SHORT,
                "waveform of %lld samples gives a negative frame count (reference raises ValueError)", (long long)n_samples);
    MLA_REQUIRE(cols <= logmel_timeline::kMaxCols, MLA_E_SHAPE, "%lld columns are more than one recording may have (%lld)", (long long)cols,
                (long long)logmel_timeline::kMaxCols);
    if (windows) *windows = W;
    if (slots) *slots = S;
    if (samples_read) *samples_read = logmel_timeline::samples_read(spec);
    return MLA_OK;
}

extern "C" int mla_logmel_timeline(const void* pcm, int pcm_dtype, int64_t recordings, int64_t n_samples, int64_t row_stride,
                                   const int64_t* desc, const int64_t* host_desc, int64_t total_slots, const float* tables, void* out,
                                   int out_dtype, mla_stream_t stream) {
    static_assert(sizeof(logmel_timeline::Rec) == logmel_timeline::kRecFields * sizeof(int64_t), "a descriptor is five int64");
    MLA_REQUIRE(recordings >= 0 && n_samples >= 0 && row_stride >= n_samples && total_slots >= 0, MLA_E_ARG,
                "bad recordings %lld / stride %lld < n_samples %lld / total_slots %lld", (long long)recordings, (long long)row_stride,
                (long long)n_samples, (long long)total_slots);
    if (const int bad = check_dtypes(pcm_dtype, out_dtype, true); bad != MLA_OK) return bad;
    if (recordings == 0) {
        MLA_REQUIRE(total_slots == 0, MLA_E_ARG, "no recordings but %lld slots", (long long)total_slots);
        return MLA_OK;
    }
    MLA_REQUIRE(pcm && desc && host_desc && tables && out, MLA_E_ARG, "null pcm/desc/host_desc/tables/out");
    if (const int bad = check_pointers(pcm, pcm_dtype, tables, out, "tables must be 4-byte and desc 8-byte aligned"); bad != MLA_OK) return bad;
    MLA_REQUIRE(mla::aligned(desc, 8), MLA_E_ARG, "tables must be 4-byte and desc 8-byte aligned");
    MLA_REQUIRE(recordings <= 0x7fffffff / logmel_timeline::kWindowItems, MLA_E_SHAPE, "too many recordings for one launch (%lld)",
                (long long)recordings);
    const logmel_timeline::Rec* recs = reinterpret_cast<const logmel_timeline::Rec*>(host_desc);
    int64_t slot_prefix = 0, item_prefix = 0;
    for (int64_t i = 0; i < recordings; ++i) {
        const logmel_timeline::Rec& r = recs[i];
        const int bad = logmel_timeline::check_rec(r, n_samples, slot_prefix, item_prefix);
        MLA_REQUIRE(bad != 1, MLA_E_ARG, "recording %lld: hop_slots %lld is not in 1 .. %lld", (long long)i, (long long)r.q,
                    (long long)logmel_timeline::kMaxCols);
        MLA_REQUIRE(bad != 2 && bad != 3, MLA_E_ARG, "recording %lld: %lld columns (%lld with a spectrum) at hop_slots %lld are no track",
                    (long long)i, (long long)r.cols, (long long)r.spec_cols, (long long)r.q);
        MLA_REQUIRE(bad != 4, MLA_E_SHAPE, "recording %lld: %lld columns read %lld samples, the rows hold %lld", (long long)i,
                    (long long)r.spec_cols, (long long)logmel_timeline::samples_read(r.spec_cols), (long long)n_samples);
        MLA_REQUIRE(bad == 0, MLA_E_ARG, "recording %lld: first_slot %lld / first_item %lld are not the sums before it (%lld / %lld)",
                    (long long)i, (long long)r.first_slot, (long long)r.first_item, (long long)slot_prefix, (long long)item_prefix);
        slot_prefix += logmel_timeline::slots_of(r.cols, r.q);
        item_prefix += logmel_timeline::items_of(r.cols, r.q);
        MLA_REQUIRE(item_prefix <= 0x7fffffff, MLA_E_SHAPE, "too many columns for one launch (%lld items at recording %lld)",
                    (long long)item_prefix, (long long)i);
    }
    MLA_REQUIRE(slot_prefix == total_slots, MLA_E_ARG, "the descriptors fill %lld slots, out has %lld", (long long)slot_prefix,
                (long long)total_slots);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_dtypes(pcm_dtype, out_dtype, pcm, row_stride, [&](auto in, auto o, auto vec) {
        using InT = decltype(in);
        using OutT = decltype(o);
        return launch_persistent(logmel_timeline_kernel<InT, OutT, decltype(vec)::value>, "logmel_timeline_kernel", kThreadsDyn, 1, kLdsBytesDyn,
                                 item_wgs(item_prefix), s, static_cast<const InT*>(pcm), row_stride, reinterpret_cast<const logmel_timeline::Rec*>(desc),
                                 int(recordings), int(item_prefix), tables, static_cast<OutT*>(out));
    });
}

extern "C" int mla_logmel_conv1(const void* pcm, int pcm_dtype, int64_t n_wave, int64_t n_samples, int64_t wave_stride,
                                const float* tables, const float* w, const float* bias, void* out, mla_stream_t stream) {
    MLA_REQUIRE(n_wave >= 0 && wave_stride >= n_samples, MLA_E_ARG, "bad n_wave %lld / stride %lld < n_samples %lld",
                (long long)n_wave, (long long)wave_stride, (long long)n_samples);
    int64_t frames = 0, examples = 0;
    const int rc = mla_logmel_counts(n_samples, &frames, &examples);
    if (rc != MLA_OK) return rc;
    if (n_wave == 0 || examples == 0) return MLA_OK;
    MLA_REQUIRE(pcm && tables && w && bias && out, MLA_E_ARG, "null pcm/tables/w/bias/out");
    if (const int bad = check_dtypes(pcm_dtype, MLA_BF16, false); bad != MLA_OK) return bad;
    if (const int bad = check_pointers(pcm, pcm_dtype, tables, out, "out must be 16-byte aligned"); bad != MLA_OK) return bad;
    MLA_REQUIRE(mla::aligned(w, 4) && mla::aligned(bias, 4), MLA_E_ARG, "out must be 16-byte aligned");
    const int64_t n_clips = n_wave * examples;
    MLA_REQUIRE(n_clips <= 0x7fffffff / kClipItems, MLA_E_SHAPE, "too many clips for one launch (%lld)", (long long)n_clips);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_pcm(pcm_dtype, pcm, wave_stride, [&](auto in, auto vec) {
        using InT = decltype(in);
        return launch_persistent(logmel_conv1_kernel<InT, decltype(vec)::value>, "logmel_conv1_kernel", kThreadsDyn, 1, kLdsBytesFused, n_clips, s,
                                 static_cast<const InT*>(pcm), wave_stride, int(examples), int(n_clips), tables, w, bias,
                                 static_cast<mma::bf16_t*>(out));
    });
}
