// conv1_core.h -- the per-pooled-row body of the bf16 patch-GEMM conv1 (conv + bias + ReLU + 2x2 max-pool as a K = 16 GEMM over
// 4 x 4 input patches; the derivation is at conv1_patch_kernel in conv.hip), shared by the stand-alone kernel (conv.hip) and the
// fused front-end (logmel.hip: log-mel rows go straight from LDS into this body). One copy, so both produce the same bits.
//
// Staged input layout (LDS, bf16): rows of kPitch = 68 elements, element (gy, gx) of the clip at column gx + 1, columns 0 and 65
// are the zero halo, as are rows outside the clip. A pooled row reads four consecutive staged rows.
#ifndef MLA_CONV1_CORE_H
#define MLA_CONV1_CORE_H

#include "mma_core.h"
#include "nanprop.h"

#ifndef MLA_CONV_NT_STORE
#define MLA_CONV_NT_STORE 1              // streaming outputs (conv epilogues, conv1) as non-temporal stores: conv1 0.43 -> 0.38 ms, conv3 -4 % in the pipeline
#endif

#ifndef MLA_CONV1_MASK_INF
#define MLA_CONV1_MASK_INF 1             // 0: without the masked form for patches that hold an Inf or NaN (A/B: what the check costs)
#endif

namespace conv1 {

using namespace mma;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kPitch = 68;                                  // bf16 per staged input row: 66 used
constexpr int kStageRow = 64 * 2 + 16;                      // bytes per pooled pixel in a wave's output stage (32 pixels)
constexpr int kStageBytes = 32 * kStageRow;

// A operand of one (position, 32-channel tile): W'[pos][channel(rho)][8 h + j] for rho = lane & 31, h = lane >> 5. The weight
// rows are permuted (MFMA row rho holds channel 16 ((rho >> 2) & 1) + (rho & 3) + 4 (rho >> 3) of its 32) so that a lane ends up
// with 16 consecutive channels of its pixel.
__device__ __forceinline__ bf16x8 weight_frag(const float* __restrict__ w, int pos, int mt, int lane) {
    const int rho = lane & 31, h = lane >> 5;
    const int chl = 16 * ((rho >> 2) & 1) + (rho & 3) + 4 * (rho >> 3);
    const int dy = pos >> 1, dx = pos & 1;
    const int ch = mt * 32 + chl;
    uint32_t pk[4];
    _Pragma("unroll") for (int jj = 0; jj < 4; ++jj) {
        float v[2];
        _Pragma("unroll") for (int e = 0; e < 2; ++e) {
            const int k = 8 * h + 2 * jj + e, i = k >> 2, c = k & 3;          // patch row i, column c
            const int ky = i - dy, kx = c - dx;
            v[e] = (ky >= 0 && ky < 3 && kx >= 0 && kx < 3) ? w[ch * 9 + ky * 3 + kx] : 0.f;
        }
        pk[jj] = pack_bf16x2(v[0], v[1]);
    }
    return __builtin_bit_cast(bf16x8, u32x4{pk[0], pk[1], pk[2], pk[3]});
}

// C/D: lane (col = pixel, hi = h) register reg <-> MFMA row (reg & 3) + 8 (reg >> 2) + 4 hi <-> channel 16 hi + reg of the tile.
// Accumulators start at the bias (max commutes with + b). `bias` may be global or LDS.
__device__ __forceinline__ f32x16 bias_frag(const float* bias, int mt, int lane) {
    f32x16 b;
    _Pragma("unroll") for (int reg = 0; reg < 16; ++reg) b[reg] = bias[mt * 32 + 16 * (lane >> 5) + reg];
    return b;
}

// One pooled row (32 pixels x 64 channels) by one wave. rows: staged input row 2 p - 1 of pooled row p (four rows are read);
// stage: kStageBytes of LDS owned by this wave; gdst: the pooled row in the NHWC output (4 KiB contiguous).
// B operand: patch rows 2h, 2h+1 of the lane's pixel, columns 2 px .. 2 px + 3 = two ds_read2_b32; 8 MFMAs; max over the four
// positions; ReLU; pack; 128-byte lines leave through the stage as non-temporal stores.
__device__ __forceinline__ void pooled_row(const uint16_t* rows, const bf16x8 (&wa)[4][2], const f32x16 (&binit)[2], char* stage,
                                           char* gdst, int lane) {
    const int px = lane & 31, h = lane >> 5;
    const uint32_t* r0 = reinterpret_cast<const uint32_t*>(rows + (2 * h) * kPitch) + px;       // 2 px bf16 = px dwords
    const uint32_t* r1 = reinterpret_cast<const uint32_t*>(rows + (2 * h + 1) * kPitch) + px;
    const u32x4 braw = u32x4{r0[0], r0[1], r1[0], r1[1]};
    const bf16x8 bfrag = __builtin_bit_cast(bf16x8, braw);
    // The four positions share ONE patch operand, and each position's filter copy is zero where it does not use a patch element:
    // 0 * inf (or 0 * NaN) = NaN would reach a position that never reads that element. A wave whose patches hold an Inf or NaN
    // (exponent all ones: the add carries into the half's bit 15) takes the masked form below -- one operand per position with the
    // unused elements zeroed, so that inf * w, relu and the pool see what nn.Conv2d's would. Wave-uniform; finite data never enters.
    const uint32_t carry = (((braw.x & 0x7fff7fffu) + 0x00800080u) | ((braw.y & 0x7fff7fffu) + 0x00800080u) |
                            ((braw.z & 0x7fff7fffu) + 0x00800080u) | ((braw.w & 0x7fff7fffu) + 0x00800080u)) & 0x80008000u;
    const bool special = MLA_CONV1_MASK_INF && __builtin_amdgcn_ballot_w64(carry != 0u) != 0ull;
    _Pragma("unroll") for (int mt = 0; mt < 2; ++mt) {
        f32x16 m;
        if (__builtin_expect(special, 0)) {
            _Pragma("unroll") for (int pos = 0; pos < 4; ++pos) {
                const int dy = pos >> 1, dx = pos & 1;                          // the position reads patch rows dy .. dy + 2, columns dx .. dx + 2
                const uint32_t c01 = dx ? 0xffff0000u : 0xffffffffu, c23 = dx ? 0xffffffffu : 0x0000ffffu;      // (col 0 | col 1 << 16), (col 2 | col 3 << 16)
                const uint32_t k0 = (2 * h >= dy && 2 * h <= dy + 2) ? 0xffffffffu : 0u, k1 = (2 * h + 1 >= dy && 2 * h + 1 <= dy + 2) ? 0xffffffffu : 0u;
                const bf16x8 bm = __builtin_bit_cast(bf16x8, u32x4{braw.x & c01 & k0, braw.y & c23 & k0, braw.z & c01 & k1, braw.w & c23 & k1});
                const f32x16 a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[pos][mt], bm, binit[mt], 0, 0, 0);
                if (pos == 0) m = a;
                else _Pragma("unroll") for (int reg = 0; reg < 16; ++reg) m[reg] = mla::nan_max(m[reg], a[reg]);
            }
        } else {
            m = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[0][mt], bfrag, binit[mt], 0, 0, 0);
            _Pragma("unroll") for (int pos = 1; pos < 4; ++pos) {
                const f32x16 a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[pos][mt], bfrag, binit[mt], 0, 0, 0);
                _Pragma("unroll") for (int reg = 0; reg < 16; ++reg) m[reg] = mla::nan_max(m[reg], a[reg]);
            }
        }
        uint32_t pk[8];
        _Pragma("unroll") for (int e = 0; e < 8; ++e) pk[e] = pack_bf16x2(mla::nan_relu(m[2 * e]), mla::nan_relu(m[2 * e + 1]));
        char* dst = stage + px * kStageRow + (mt * 32 + 16 * h) * 2;              // 16 consecutive channels of pixel px
        *reinterpret_cast<u32x4*>(dst) = u32x4{pk[0], pk[1], pk[2], pk[3]};
        *reinterpret_cast<u32x4*>(dst + 16) = u32x4{pk[4], pk[5], pk[6], pk[7]};
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the stage rows belong to this wave only:
    __builtin_amdgcn_wave_barrier();                            // LDS operations of one wave execute in order
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    _Pragma("unroll") for (int it = 0; it < 4; ++it) {                      // 32 pixels x 128 B = 4 KiB contiguous per wave
        const int piece = it * 64 + lane, p = piece >> 3, c = piece & 7;
#if MLA_CONV_NT_STORE
        __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(stage + p * kStageRow + c * 16), reinterpret_cast<u32x4*>(gdst + size_t(piece) * 16));
#else
        *reinterpret_cast<u32x4*>(gdst + size_t(piece) * 16) = *reinterpret_cast<const u32x4*>(stage + p * kStageRow + c * 16);
#endif
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the reads above precede the next row's stage writes
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace conv1
#endif
