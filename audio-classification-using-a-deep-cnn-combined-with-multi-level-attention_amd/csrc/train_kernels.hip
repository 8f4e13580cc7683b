// train_kernels.hip -- the remaining pieces of the reference's inner training step
// (train.py:124-138): cross-entropy on the sigmoid scores (train.py:372 nn.CrossEntropyLoss,
// mean reduction, applied on top of model.py:268's sigmoid outputs), helpers for the Linear
// backward (transposes feeding the MFMA GEMM, column sums for bias gradients), and the Adam
// update (train.py:369 optim.Adam: betas 0.9/0.999, eps 1e-8, no weight decay, no amsgrad) over
// one flat parameter buffer. The helpers come in f32 and bf16 (the bf16 finetune step's Linear layers).
#include "adam_groups.h"
#include "ce_core.h"
#include "common.h"
#include "mma_core.h"

namespace {

using mma::bf16_t;

// out[c][r] = in[r][c]; 32x32 tiles through LDS (padded against bank conflicts)
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, int64_t ld_in, float* __restrict__ out,
                                                        int64_t ld_out, int64_t rows, int64_t cols) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8
    const int64_t c0 = int64_t(blockIdx.x) * 32, r0 = int64_t(blockIdx.y) * 32;
    _Pragma("unroll") for (int j = 0; j < 32; j += 8) {
        const int64_t r = r0 + ty + j, c = c0 + tx;
        if (r < rows && c < cols) tile[ty + j][tx] = in[r * ld_in + c];
    }
    __syncthreads();
    _Pragma("unroll") for (int j = 0; j < 32; j += 8) {
        const int64_t c = c0 + ty + j, r = r0 + tx;
        if (r < rows && c < cols) out[c * ld_out + r] = tile[tx][ty + j];
    }
}

// out[c][r] = in[r][c] for 2-byte elements; 64 x 64 tiles through LDS
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const uint16_t* __restrict__ in, int64_t ld_in, uint16_t* __restrict__ out,
                                                             int64_t ld_out, int64_t rows, int64_t cols) {
    __shared__ uint16_t tile[64][66];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;          // 64 x 4
    const int64_t c0 = int64_t(blockIdx.x) * 64, r0 = int64_t(blockIdx.y) * 64;
    _Pragma("unroll") for (int j = 0; j < 64; j += 4) {
        const int64_t r = r0 + ty + j, c = c0 + tx;
        tile[ty + j][tx] = (r < rows && c < cols) ? in[r * ld_in + c] : uint16_t(0);
    }
    __syncthreads();
    _Pragma("unroll") for (int j = 0; j < 64; j += 4) {
        const int64_t c = c0 + ty + j, r = r0 + tx;
        if (c < cols && r < ld_out) out[c * ld_out + r] = r < rows ? tile[tx][ty + j] : uint16_t(0);     // zero the row padding too
    }
}

// loss = inv_total * sum_b (logsumexp(x_b) - x_b[y_b]);  dx = inv_total * (softmax(x_b) - onehot(y_b))
// one block: deterministic double-precision reduction. inv_total = 1 / (global batch).
// A label outside [0, K) (nn.CrossEntropyLoss raises "Target out of bounds" for it) is never used as an index: the row
// contributes nothing, the loss comes out NaN and n_correct[1] = the number of such labels, which the host layer turns into
// the exception (ops.cross_entropy / train_model) without a per-step synchronisation of its own.
__global__ __launch_bounds__(256) void cross_entropy_kernel(const float* __restrict__ x, int64_t ldx,
                                                            const int64_t* __restrict__ labels, int64_t rows, int K,
                                                            float inv_total, float* __restrict__ loss, float* __restrict__ dx,
                                                            int64_t ld_dx, int* __restrict__ n_correct) {
    __shared__ double part[256];
    __shared__ int hits[256];
    __shared__ int bads[256];
    double acc = 0.0;
    int correct = 0, bad = 0;
    for (int64_t b = threadIdx.x; b < rows; b += 256) {
        const float* row = x + b * ldx;
        float mx = row[0];
        int arg = 0;
        for (int k = 1; k < K; ++k)
            if (row[k] > mx) { mx = row[k]; arg = k; }
        float den = 0.f;
        for (int k = 0; k < K; ++k) den += __expf(row[k] - mx);
        const float lse = mx + __logf(den);
        const int64_t y64 = labels[b];
        const bool ok = y64 >= 0 && y64 < K;
        const int y = ok ? int(y64) : -1;
        bad += !ok;
        if (ok) acc += double(lse - row[y]);
        correct += (arg == y);
        if (dx)
            for (int k = 0; k < K; ++k) dx[b * ld_dx + k] = ok ? (__expf(row[k] - lse) - (k == y ? 1.f : 0.f)) * inv_total : 0.f;
    }
    part[threadIdx.x] = acc;
    hits[threadIdx.x] = correct;
    bads[threadIdx.x] = bad;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            part[threadIdx.x] += part[threadIdx.x + o];
            hits[threadIdx.x] += hits[threadIdx.x + o];
            bads[threadIdx.x] += bads[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *loss = bads[0] ? __builtin_nanf("") : float(part[0] * inv_total);
        if (n_correct) { n_correct[0] = hits[0]; n_correct[1] = bads[0]; }
    }
}

// ---- nn.CrossEntropyLoss with class weights, label smoothing and ignore_index (formulas and lane layout: ce_core.h) ----
// Three launches, no floating-point atomics and none on integers either: the denominator of the mean (labels and weights only, so
// a data-parallel step can all-reduce it in front of the loss), one wavefront per row, and one workgroup that adds the row terms
// and the row flags in a fixed order. The scale 1 / den is read from device memory: the sequence replays in a HIP graph.
template <typename T>
__device__ __forceinline__ T block_tree_256(T v, T* part) {
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    const T r = part[0];
    __syncthreads();                                        // part is used again
    return r;
}

__global__ __launch_bounds__(ce::kThreads) void cross_entropy_den_kernel(const int64_t* __restrict__ labels, int64_t rows, int K,
                                                                         const float* __restrict__ w, int64_t ignore_index,
                                                                         float* __restrict__ den) {
    __shared__ double part[ce::kThreads];
    const double s = block_tree_256(ce::den_thread(labels, rows, K, w, ignore_index, threadIdx.x), part);
    if (threadIdx.x == 0) den[0] = float(s);
}

__device__ __forceinline__ ce::MaxAt wave_max_at(ce::MaxAt v) {
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) v = ce::max_combine(v, ce::MaxAt{__shfl_xor(v.m, o), __shfl_xor(v.i, o)});
    return v;
}

__device__ __forceinline__ float wave_sum_f32(float v) {
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void cross_entropy_opts_kernel(const float* __restrict__ x, int64_t ldx, const int64_t* __restrict__ labels,
                                                                 int64_t rows, int K, const float* __restrict__ w, int64_t ignore_index,
                                                                 float smoothing, const float* __restrict__ den, float* __restrict__ dx,
                                                                 int64_t ld_dx, double* __restrict__ term, int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t b = int64_t(blockIdx.x) * ce::kRowsPerWg + (threadIdx.x >> 6);
    if (b >= rows) return;                                  // the whole wave; no barrier below
    const int64_t y64 = labels[b];
    const int cls = ce::classify(y64, K, ignore_index);
    if (cls != ce::kCounted) {                              // ignored, or a label that must not be used as an index: zeros, no loss
        if (dx)
            for (int k = lane; k < K; k += ce::kLanes) dx[b * ld_dx + k] = 0.f;
        if (lane == 0) { term[b] = 0.0; flags[b] = cls; }
        return;
    }
    const float* row = x + b * ldx;
    float xv[ce::kPerLane];
    _Pragma("unroll") for (int j = 0; j < ce::kPerLane; ++j) {
        const int k = lane + ce::kLanes * j;
        xv[j] = k < K ? row[k] : 0.f;
    }
    const ce::MaxAt top = wave_max_at(ce::lane_max(xv, K, lane));
    ce::Row r;
    r.y = int(y64);
    r.lse = top.m + ce::fast_log(wave_sum_f32(ce::lane_sum_exp(xv, K, lane, top.m)));
    r.c = (1.f - smoothing) * (w ? w[r.y] : 1.f);
    r.ek = smoothing / float(K);
    r.wsum = 0.f;
    r.s = den ? 1.f / den[0] : 1.f;
    float t = 0.f;
    if (r.ek > 0.f) {
        ce::lane_smooth(xv, w, K, lane, r.lse, &t, &r.wsum);
        t = wave_sum_f32(t);
        r.wsum = wave_sum_f32(r.wsum);
    }
    if (dx) {
        _Pragma("unroll") for (int j = 0; j < ce::kPerLane; ++j) {
            const int k = lane + ce::kLanes * j;
            if (k < K) dx[b * ld_dx + k] = ce::dx_elem(r, xv[j], k, (w && r.ek > 0.f) ? w[k] : 1.f);
        }
    }
    if (lane == 0) {
        term[b] = ce::row_loss(r, row[r.y], t);
        flags[b] = ce::kCounted | (top.i == r.y ? ce::kHit : 0);
    }
}

__global__ __launch_bounds__(ce::kThreads) void cross_entropy_finish_kernel(const double* __restrict__ term, const int32_t* __restrict__ flags,
                                                                            int64_t rows, int reduction, const float* __restrict__ den,
                                                                            float* __restrict__ loss, int* __restrict__ counts) {
    __shared__ double part[ce::kThreads];
    __shared__ int ipart[ce::kThreads];
    int n3[3];
    const double s = block_tree_256(ce::finish_thread(term, flags, rows, threadIdx.x, n3), part);
    _Pragma("unroll") for (int i = 0; i < 3; ++i) n3[i] = block_tree_256(n3[i], ipart);
    if (threadIdx.x == 0) {
        *loss = ce::finish_loss(s, n3[1], reduction, den);
        counts[0] = n3[0]; counts[1] = n3[1]; counts[2] = n3[2];
    }
}

// column sums of a (rows, cols) f32 | bf16 matrix: block (x = 64-column tile, y = row chunk) -> partials
template <typename T>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const T* __restrict__ x, int64_t ldx, int64_t rows, int cols,
                                                             double* __restrict__ partial) {
    __shared__ double part[4][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int64_t per = (rows + gridDim.y - 1) / gridDim.y;
    const int64_t r0 = int64_t(blockIdx.y) * per, r1 = r0 + per < rows ? r0 + per : rows;
    double s = 0.0;
    if (c < cols)
        for (int64_t r = r0 + g; r < r1; r += 4) s += double(mma::load_elem(x + r * ldx + c));
    part[g][lane] = s;
    __syncthreads();
    if (g == 0 && c < cols) partial[int64_t(blockIdx.y) * cols + c] = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
}

// the same with 16-byte loads: thread (row group g, column quad q) of block (x = 256-column tile, y = row chunk) adds the four
// columns 4 q .. 4 q + 3 of rows g, g + 4, ... of the chunk; a wave reads 1 KiB of one row per instruction (the scalar form: 256 B)
__global__ __launch_bounds__(256) void colsum_partial4_kernel(const float* __restrict__ x, int64_t ldx, int64_t rows, int cols,
                                                              double* __restrict__ partial) {
    __shared__ double part[4][64][4];
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * 4;
    const int64_t per = (rows + gridDim.y - 1) / gridDim.y;
    const int64_t r0 = int64_t(blockIdx.y) * per, r1 = r0 + per < rows ? r0 + per : rows;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (c < cols)
        for (int64_t r = r0 + g; r < r1; r += 4) {
            const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + r * ldx + c);
            s0 += v.x; s1 += v.y; s2 += v.z; s3 += v.w;
        }
    part[g][lane][0] = s0; part[g][lane][1] = s1; part[g][lane][2] = s2; part[g][lane][3] = s3;
    __syncthreads();
    if (g == 0 && c < cols)
        _Pragma("unroll") for (int e = 0; e < 4; ++e)
            partial[int64_t(blockIdx.y) * cols + c + e] = part[0][lane][e] + part[1][lane][e] + part[2][lane][e] + part[3][lane][e];
}

__global__ void colsum_finish_kernel(const double* __restrict__ partial, int chunks, int cols, float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += partial[int64_t(k) * cols + c];
    out[c] = float(s);
}

__global__ void axpy_kernel(float a, const float* __restrict__ x, float* __restrict__ y, int64_t n) {
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) y[i] += a * x[i];
}

// torch.optim.Adam single-tensor step (no weight decay, no amsgrad):
//   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// One update function for both kernel forms, with the fused multiply-adds written out and contraction off: left to the
// compiler, `b1 * m + (1 - b1) * g` fuses around either product, and it chose differently in the two kernels (last-bit
// differences between an eager step and its graph replay).
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, int64_t i, float b1, float b2, float eps, float step_size,
                                            float inv_sqrt_bc2) {
#pragma clang fp contract(off)
    const float gi = g[i];
    const float mi = fmaf(b1, m[i], (1.f - b1) * gi);
    const float vi = fmaf(b2, v[i], (1.f - b2) * (gi * gi));
    m[i] = mi;
    v[i] = vi;
    const float den = fmaf(sqrtf(vi), inv_sqrt_bc2, eps);
    p[i] = p[i] - step_size * mi / den;
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            int64_t n, float b1, float b2, float eps, float step_size, float inv_sqrt_bc2) {
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
        adam_update(p, g, m, v, i, b1, b2, eps, step_size, inv_sqrt_bc2);
}

// The same step with its two step-dependent scalars (lr / (1 - b1^t), 1 / sqrt(1 - b2^t)) read from device memory: a HIP graph
// that holds this launch replays with the values of the moment, which mla_adam_prepare writes (computed on the host exactly as
// mla_adam_step computes them, so both forms update the parameters bit for bit alike).
__global__ void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                int64_t n, float b1, float b2, float eps, const float* __restrict__ scal) {
    const float step_size = scal[0], inv_sqrt_bc2 = scal[1];
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
        adam_update(p, g, m, v, i, b1, b2, eps, step_size, inv_sqrt_bc2);
}

__global__ void set2_kernel(float* dst, float a, float b) { dst[0] = a; dst[1] = b; }

// ---- the grouped step: torch.optim.Adam / AdamW with parameter groups over the same flat buffers, ONE launch for all groups ----
// Which group owns a quad of four elements comes from the table of adam_groups.h (one lookup per workgroup chunk, then a walk
// along the runs the chunk crosses); what the group asks for from its row of `groups` (mla_adam_groups_prepare). adam_update's
// arithmetic, on values, extended by what torch's single-tensor step does around it -- with every option off the same operations
// in the same order, so the same bits:
//   g <- coef g (clip_grad_norm_'s factor, read from device memory; g itself is not written back)
//   g <- g + wd p (L2) | p <- p (1 - lr wd) (decoupled) ; m, v as before ; vmax <- max(vmax, v) and sqrt(vmax) in the denominator (amsgrad)
struct GroupRow { float step_size, inv_sqrt_bc2, b1, b2, eps, decay; int flags; };

__device__ __forceinline__ GroupRow load_group(const float* __restrict__ groups, int64_t grp) {
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(groups + grp * adam_groups::kGroupFloats);
    const f32x4_t b = *reinterpret_cast<const f32x4_t*>(groups + grp * adam_groups::kGroupFloats + 4);
    return GroupRow{a.x, a.y, a.z, a.w, b.x, b.y, int(b.z)};
}

__device__ __forceinline__ void adam_update_ext(float& p, float g, float& m, float& v, float& vmax, const GroupRow& s, bool ams, bool clip, float coef) {
#pragma clang fp contract(off)
    float gi = g;
    if (clip) gi = coef * gi;
    if (s.flags & adam_groups::kL2) gi = gi + s.decay * p;
    float pi = p;
    if (s.flags & adam_groups::kDecoupled) pi = pi * s.decay;
    const float mi = fmaf(s.b1, m, (1.f - s.b1) * gi);
    const float vi = fmaf(s.b2, v, (1.f - s.b2) * (gi * gi));
    m = mi;
    v = vi;
    float vd = vi;
    if (ams) {
        vd = (vi > vmax || vi != vi) ? vi : vmax;               // torch.maximum: a NaN stays
        vmax = vd;
    }
    const float den = fmaf(sqrtf(vd), s.inv_sqrt_bc2, s.eps);
    p = pi - s.step_size * mi / den;
}

__global__ __launch_bounds__(256) void adam_grouped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, float* __restrict__ vmax, int64_t n,
                                                           const int64_t* __restrict__ table, int64_t n_runs, int64_t n_chunks, int64_t n_pads,
                                                           const float* __restrict__ groups, int n_groups, const float* __restrict__ coef_dev) {
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    const int64_t* run_end = table;
    const int64_t* run_group = run_end + n_runs;
    const int64_t* chunk_run = run_group + n_runs;
    const int64_t* chunk_pad = chunk_run + n_chunks;
    const int64_t* pad = chunk_pad + n_chunks + 1;
    const bool clip = coef_dev != nullptr;
    const float coef = clip ? *coef_dev : 1.f;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        // every index read from the table is clamped to its section: whatever the table holds, no access leaves the buffers
        int64_t r0 = chunk_run[c];
        r0 = r0 < 0 ? 0 : (r0 >= n_runs ? n_runs - 1 : r0);
        int64_t pad0 = chunk_pad[c], pad1 = chunk_pad[c + 1];
        pad0 = pad0 < 0 ? 0 : (pad0 > n_pads ? n_pads : pad0);
        pad1 = pad1 < pad0 ? pad0 : (pad1 > n_pads ? n_pads : pad1);
        // the chunk's data first (nothing in it depends on the table), then the walk along the runs: the table's dependent loads
        // run under the data's latency instead of in front of it (at the head's 0.8 M elements that chain was a fifth of the launch)
        constexpr int kQuads = adam_groups::kAdamChunk / 1024;
        const int64_t q0 = c * adam_groups::kAdamChunk + int64_t(threadIdx.x) * 4;
        f32x4_t pv[kQuads], gv[kQuads], mv[kQuads], vv[kQuads];
        _Pragma("unroll") for (int u = 0; u < kQuads; ++u) {
            const int64_t q = q0 + u * 1024;
            if (q >= n) continue;                               // n is a multiple of 4
            pv[u] = *reinterpret_cast<const f32x4_t*>(p + q);
            gv[u] = *reinterpret_cast<const f32x4_t*>(g + q);
            mv[u] = *reinterpret_cast<const f32x4_t*>(m + q);
            vv[u] = *reinterpret_cast<const f32x4_t*>(v + q);
        }
        _Pragma("unroll") for (int u = 0; u < kQuads; ++u) {
            const int64_t q = q0 + u * 1024;
            if (q >= n) continue;
            int64_t r = r0;
            while (r + 1 < n_runs && q >= run_end[r]) ++r;
            int64_t grp = run_group[r];
            grp = grp < 0 ? 0 : (grp >= n_groups ? n_groups - 1 : grp);
            const GroupRow s = load_group(groups, grp);
            int valid = 4;                                      // a quad that ends a tensor of 4 k + 1 | 2 | 3 elements: the rest is padding
            for (int64_t k = pad0; k < pad1; ++k)
                if (pad[2 * k] == q) valid = int(pad[2 * k + 1]);
            const bool ams = (s.flags & adam_groups::kAmsgrad) && vmax != nullptr;   // (the launcher's callers pair the flag with the buffer)
            f32x4_t xv = {0.f, 0.f, 0.f, 0.f};
            if (ams) xv = *reinterpret_cast<const f32x4_t*>(vmax + q);
            float pe[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w}, me[4] = {mv[u].x, mv[u].y, mv[u].z, mv[u].w};
            float ve[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w}, xe[4] = {xv.x, xv.y, xv.z, xv.w};
            const float ge[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
            _Pragma("unroll") for (int e = 0; e < 4; ++e)
                if (e < valid) adam_update_ext(pe[e], ge[e], me[e], ve[e], xe[e], s, ams, clip, coef);
            *reinterpret_cast<f32x4_t*>(p + q) = f32x4_t{pe[0], pe[1], pe[2], pe[3]};
            *reinterpret_cast<f32x4_t*>(m + q) = f32x4_t{me[0], me[1], me[2], me[3]};
            *reinterpret_cast<f32x4_t*>(v + q) = f32x4_t{ve[0], ve[1], ve[2], ve[3]};
            if (ams) *reinterpret_cast<f32x4_t*>(vmax + q) = f32x4_t{xe[0], xe[1], xe[2], xe[3]};
        }
    }
}

struct GroupTable { float v[adam_groups::kMaxGroups * adam_groups::kGroupFloats]; };

__global__ __launch_bounds__(256) void set_groups_kernel(float* __restrict__ dst, GroupTable tab, int count) {
    for (int i = threadIdx.x; i < count; i += 256) dst[i] = tab.v[i];
}

// L2 norm of the flat gradient, deterministic: block b adds the squares of its quads (b, b + grid, ...) in double, lanes
// combine through LDS in a fixed tree; grid = adam_groups::norm_blocks(n), a function of n alone. The finishing block adds the
// partial sums the same way and writes [norm, coef], coef = min(1, max_norm / (norm + 1e-6)) as torch's clip_grad_norm_ forms it
// in float32 (a NaN norm gives a NaN coefficient, like torch.clamp).
__device__ __forceinline__ double block_sum_256(double acc, double* part) {
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    return part[0];
}

__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partial) {
    __shared__ double part[256];
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    double acc = 0.0;
    for (int64_t q = (int64_t(blockIdx.x) * 256 + threadIdx.x) * 4; q < n; q += int64_t(gridDim.x) * 1024) {
        if (q + 4 <= n) {
            const f32x4_t x = *reinterpret_cast<const f32x4_t*>(g + q);
            acc += double(x.x) * double(x.x); acc += double(x.y) * double(x.y);
            acc += double(x.z) * double(x.z); acc += double(x.w) * double(x.w);
        } else {
            for (int64_t i = q; i < n; ++i) acc += double(g[i]) * double(g[i]);
        }
    }
    const double s = block_sum_256(acc, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partial, int blocks, float max_norm,
                                                               float* __restrict__ out2) {
    __shared__ double part[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 256) acc += partial[i];
    const double s = block_sum_256(acc, part);
    if (threadIdx.x == 0) {
        const float norm = float(sqrt(s));
        const float c = max_norm / (norm + 1e-6f);
        out2[0] = norm;
        out2[1] = c > 1.f ? 1.f : c;
    }
}

__global__ void counter_add_kernel(int64_t* counter, int64_t delta) { *counter += delta; }

// splitmix64 finaliser; the same three lines as weights.py _mix (uint64 wrap-around arithmetic only)
__host__ __device__ inline uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// 16 mask bytes per thread and store (one dwordx4): HBM-write-bound, 1 B per element
__global__ __launch_bounds__(256) void dropout_mask_kernel(uint8_t* __restrict__ mask, int64_t n, uint64_t key, uint64_t offset,
                                                           uint32_t thresh) {
    const uint64_t gold = 0x9E3779B97F4A7C15ull;
    for (int64_t i0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * 16; i0 < n; i0 += int64_t(gridDim.x) * blockDim.x * 16) {
        uint32_t w[4] = {0, 0, 0, 0};
        _Pragma("unroll") for (int j = 0; j < 16; ++j) {
            const uint64_t z = mix64((offset + uint64_t(i0 + j)) * gold + key);
            w[j >> 2] |= uint32_t(uint32_t(z >> 40) >= thresh) << (8 * (j & 3));
        }
        if (i0 + 16 <= n && (reinterpret_cast<uintptr_t>(mask + i0) & 15) == 0) {
            *reinterpret_cast<uint4*>(mask + i0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int j = 0; j < 16 && i0 + j < n; ++j) mask[i0 + j] = uint8_t(w[j >> 2] >> (8 * (j & 3)));
        }
    }
}

// the same mask with stream_id = stream_base + *counter + 1 read on the device (graph replays draw a fresh mask per step)
__global__ __launch_bounds__(256) void dropout_mask_dev_kernel(uint8_t* __restrict__ mask, int64_t n, uint64_t seed, uint64_t stream_base,
                                                               const int64_t* __restrict__ counter, uint64_t offset, uint32_t thresh) {
    const uint64_t gold = 0x9E3779B97F4A7C15ull;
    const uint64_t key = mix64(seed * gold + stream_base + uint64_t(*counter) + 1ull);
    for (int64_t i0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * 16; i0 < n; i0 += int64_t(gridDim.x) * blockDim.x * 16) {
        uint32_t w[4] = {0, 0, 0, 0};
        _Pragma("unroll") for (int j = 0; j < 16; ++j) {
            const uint64_t z = mix64((offset + uint64_t(i0 + j)) * gold + key);
            w[j >> 2] |= uint32_t(uint32_t(z >> 40) >= thresh) << (8 * (j & 3));
        }
        if (i0 + 16 <= n && (reinterpret_cast<uintptr_t>(mask + i0) & 15) == 0) {
            *reinterpret_cast<uint4*>(mask + i0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int j = 0; j < 16 && i0 + j < n; ++j) mask[i0 + j] = uint8_t(w[j >> 2] >> (8 * (j & 3)));
        }
    }
}

unsigned grid_for(int64_t n) { return unsigned((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192); }

}  // namespace

extern "C" int mla_transpose_f32(const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t rows, int64_t cols,
                                 mla_stream_t stream) {
    MLA_REQUIRE(in && out && rows > 0 && cols > 0 && ld_in >= cols && ld_out >= rows, MLA_E_ARG, "bad transpose arguments");
    hipLaunchKernelGGL(transpose_kernel, dim3(unsigned((cols + 31) / 32), unsigned((rows + 31) / 32)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), in, ld_in, out, ld_out, rows, cols);
    MLA_LAUNCH_OK("transpose");
    return MLA_OK;
}

extern "C" int mla_transpose_bf16(const void* in, int64_t ld_in, void* out, int64_t ld_out, int64_t rows, int64_t cols,
                                  mla_stream_t stream) {
    MLA_REQUIRE(in && out && rows > 0 && cols > 0 && ld_in >= cols && ld_out >= rows, MLA_E_ARG, "bad transpose arguments");
    hipLaunchKernelGGL(transpose_bf16_kernel, dim3(unsigned((cols + 63) / 64), unsigned((ld_out + 63) / 64)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<const uint16_t*>(in), ld_in, static_cast<uint16_t*>(out), ld_out, rows, cols);
    MLA_LAUNCH_OK("transpose_bf16");
    return MLA_OK;
}

extern "C" int mla_cross_entropy(const float* x, int64_t ldx, const int64_t* labels, int64_t rows, int K, float inv_total,
                                 float* loss, float* dx, int64_t ld_dx, int* n_correct, mla_stream_t stream) {
    MLA_REQUIRE(x && labels && loss && rows > 0 && K >= 1 && ldx >= K, MLA_E_ARG, "bad cross_entropy arguments");
    hipLaunchKernelGGL(cross_entropy_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), x, ldx, labels, rows, K,
                       inv_total, loss, dx, ld_dx, n_correct);
    MLA_LAUNCH_OK("cross_entropy");
    return MLA_OK;
}

extern "C" int mla_cross_entropy_den(const int64_t* labels, int64_t rows, int K, const float* weight, int64_t ignore_index, float* den,
                                     mla_stream_t stream) {
    MLA_REQUIRE(labels && den, MLA_E_ARG, "cross_entropy_den: null labels or den");
    MLA_REQUIRE(rows > 0, MLA_E_ARG, "cross_entropy_den: rows = %lld", (long long)rows);
    MLA_REQUIRE(K >= 1 && K <= ce::kMaxK, MLA_E_SHAPE, "cross_entropy_den: K = %d, built for 1 to %d classes", K, ce::kMaxK);
    hipLaunchKernelGGL(cross_entropy_den_kernel, dim3(1), dim3(ce::kThreads), 0, static_cast<hipStream_t>(stream), labels, rows, K, weight,
                       ignore_index, den);
    MLA_LAUNCH_OK("cross_entropy_den");
    return MLA_OK;
}

extern "C" int64_t mla_cross_entropy_opts_workspace_bytes(int64_t rows) { return ce::workspace_bytes(rows); }

extern "C" int mla_cross_entropy_opts(const float* x, int64_t ldx, const int64_t* labels, int64_t rows, int K, const float* weight,
                                      int64_t ignore_index, float label_smoothing, int reduction, const float* den, float* loss, float* dx,
                                      int64_t ld_dx, int* counts, void* workspace, mla_stream_t stream) {
    MLA_REQUIRE(x && labels && loss && counts && workspace, MLA_E_ARG, "cross_entropy_opts: null x, labels, loss, counts or workspace");
    MLA_REQUIRE(rows > 0, MLA_E_ARG, "cross_entropy_opts: rows = %lld", (long long)rows);
    MLA_REQUIRE(K >= 1 && K <= ce::kMaxK, MLA_E_SHAPE, "cross_entropy_opts: K = %d, built for 1 to %d classes (16 per lane of a wavefront)", K,
                ce::kMaxK);
    MLA_REQUIRE(ldx >= K && (!dx || ld_dx >= K), MLA_E_ARG, "cross_entropy_opts: a row pitch below K = %d", K);
    MLA_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, MLA_E_ARG, "cross_entropy_opts: label_smoothing %g outside [0, 1]",
                double(label_smoothing));
    MLA_REQUIRE(reduction == ce::kMean || reduction == ce::kSum, MLA_E_ARG, "cross_entropy_opts: reduction code %d (0 = mean, 1 = sum)", reduction);
    MLA_REQUIRE(reduction != ce::kMean || den, MLA_E_ARG, "cross_entropy_opts: the mean needs den (mla_cross_entropy_den)");
    MLA_REQUIRE(mla::aligned(workspace, 8), MLA_E_ARG, "cross_entropy_opts: the workspace must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* term = static_cast<double*>(workspace);
    int32_t* flags = reinterpret_cast<int32_t*>(term + rows);
    const float* scale = reduction == ce::kMean ? den : nullptr;
    hipLaunchKernelGGL(cross_entropy_opts_kernel, dim3(unsigned((rows + ce::kRowsPerWg - 1) / ce::kRowsPerWg)), dim3(256), 0, s, x, ldx, labels,
                       rows, K, weight, ignore_index, label_smoothing, scale, dx, ld_dx, term, flags);
    MLA_LAUNCH_OK("cross_entropy_opts");
    hipLaunchKernelGGL(cross_entropy_finish_kernel, dim3(1), dim3(ce::kThreads), 0, s, term, flags, rows, reduction, scale, loss, counts);
    MLA_LAUNCH_OK("cross_entropy_opts finish");
    return MLA_OK;
}

// workspace: 64 * cols doubles
extern "C" int mla_col_sum(const float* x, int64_t ldx, int64_t rows, int64_t cols, void* workspace, float* out,
                           mla_stream_t stream) {
    MLA_REQUIRE(x && workspace && out && rows > 0 && cols > 0 && ldx >= cols, MLA_E_ARG, "bad col_sum arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int chunks = int(rows / 64 < 1 ? 1 : (rows / 64 > 64 ? 64 : rows / 64));       // <= 64: the workspace
    if (cols % 4 == 0 && ldx % 4 == 0 && mla::aligned(x, 16)) {          // 16-byte loads
        hipLaunchKernelGGL(colsum_partial4_kernel, dim3(unsigned((cols + 255) / 256), unsigned(chunks)), dim3(256), 0, s, x, ldx, rows,
                           int(cols), static_cast<double*>(workspace));
    } else {                                                             // narrow matrices (the attention modules' 10 columns): rows are the parallelism
        hipLaunchKernelGGL(colsum_partial_kernel<float>, dim3(unsigned((cols + 63) / 64), unsigned(chunks)), dim3(256), 0, s, x, ldx, rows,
                           int(cols), static_cast<double*>(workspace));
    }
    MLA_LAUNCH_OK("colsum partial");
    hipLaunchKernelGGL(colsum_finish_kernel, dim3(unsigned((cols + 255) / 256)), dim3(256), 0, s,
                       static_cast<const double*>(workspace), chunks, int(cols), out);
    MLA_LAUNCH_OK("colsum finish");
    return MLA_OK;
}

// workspace: 64 * cols doubles
extern "C" int mla_col_sum_bf16(const void* x, int64_t ldx, int64_t rows, int64_t cols, void* workspace, float* out,
                                mla_stream_t stream) {
    MLA_REQUIRE(x && workspace && out && rows > 0 && cols > 0 && ldx >= cols, MLA_E_ARG, "bad col_sum arguments");
    const int chunks = int(rows / 256 < 1 ? 1 : (rows / 256 > 64 ? 64 : rows / 256));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(colsum_partial_kernel<bf16_t>, dim3(unsigned((cols + 63) / 64), unsigned(chunks)), dim3(256), 0, s,
                       static_cast<const bf16_t*>(x), ldx, rows, int(cols), static_cast<double*>(workspace));
    MLA_LAUNCH_OK("colsum partial bf16");
    hipLaunchKernelGGL(colsum_finish_kernel, dim3(unsigned((cols + 255) / 256)), dim3(256), 0, s,
                       static_cast<const double*>(workspace), chunks, int(cols), out);
    MLA_LAUNCH_OK("colsum finish bf16");
    return MLA_OK;
}

extern "C" int mla_axpy(float a, const float* x, float* y, int64_t n, mla_stream_t stream) {
    MLA_REQUIRE(x && y && n >= 0, MLA_E_ARG, "bad axpy arguments");
    if (n == 0) return MLA_OK;
    hipLaunchKernelGGL(axpy_kernel, dim3(grid_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), a, x, y, n);
    MLA_LAUNCH_OK("axpy");
    return MLA_OK;
}

extern "C" int mla_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                             float eps, int64_t step, mla_stream_t stream) {
    MLA_REQUIRE(p && g && m && v && n >= 0 && step >= 1, MLA_E_ARG, "bad adam arguments");
    if (n == 0) return MLA_OK;
    const double bc1 = 1.0 - pow(double(beta1), double(step)), bc2 = 1.0 - pow(double(beta2), double(step));
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, m, v, n, beta1, beta2,
                       eps, float(double(lr) / bc1), float(1.0 / sqrt(bc2)));
    MLA_LAUNCH_OK("adam");
    return MLA_OK;
}

extern "C" int mla_adam_prepare(float* scal2_dev, float lr, float beta1, float beta2, int64_t step, mla_stream_t stream) {
    MLA_REQUIRE(scal2_dev && step >= 1, MLA_E_ARG, "bad adam_prepare arguments");
    const double bc1 = 1.0 - pow(double(beta1), double(step)), bc2 = 1.0 - pow(double(beta2), double(step));
    hipLaunchKernelGGL(set2_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), scal2_dev, float(double(lr) / bc1),
                       float(1.0 / sqrt(bc2)));
    MLA_LAUNCH_OK("adam_prepare");
    return MLA_OK;
}

extern "C" int mla_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float beta1, float beta2, float eps,
                                 const float* scal2_dev, mla_stream_t stream) {
    MLA_REQUIRE(p && g && m && v && scal2_dev && n >= 0, MLA_E_ARG, "bad adam arguments");
    if (n == 0) return MLA_OK;
    hipLaunchKernelGGL(adam_dev_kernel, dim3(grid_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, m, v, n, beta1, beta2,
                       eps, scal2_dev);
    MLA_LAUNCH_OK("adam (scalars on the device)");
    return MLA_OK;
}

extern "C" int mla_adam_groups_table(const int64_t* numel, const int32_t* group, int64_t n_tensors, int n_groups, int64_t* table,
                                     int64_t capacity, int64_t* counts5) {
    MLA_REQUIRE(numel && group && counts5 && n_tensors >= 1, MLA_E_ARG, "bad adam_groups_table arguments");
    adam_groups::Counts c;
    const int bad = adam_groups::count(numel, group, n_tensors, n_groups, &c);
    MLA_REQUIRE(bad != 3, MLA_E_SHAPE, "%d optimizer groups: the grouped Adam step takes 1 to %d", n_groups, adam_groups::kMaxGroups);
    MLA_REQUIRE(bad == 0, MLA_E_ARG, bad == 1 ? "a tensor without elements" : "a group index outside [0, n_groups)");
    counts5[0] = c.total; counts5[1] = c.runs; counts5[2] = c.pads; counts5[3] = c.chunks; counts5[4] = c.words;
    if (!table) return MLA_OK;                                   // the sizes only
    MLA_REQUIRE(capacity >= c.words, MLA_E_ARG, "adam_groups_table: %lld words of room, %lld needed", (long long)capacity, (long long)c.words);
    adam_groups::build(numel, group, n_tensors, c, table);
    return MLA_OK;
}

extern "C" int mla_adam_groups_prepare(float* groups_dev, const mla_adam_group_t* groups, int n_groups, int64_t step, mla_stream_t stream) {
    MLA_REQUIRE(groups_dev && groups && step >= 1 && n_groups >= 1, MLA_E_ARG, "bad adam_groups_prepare arguments");
    MLA_REQUIRE(n_groups <= adam_groups::kMaxGroups, MLA_E_SHAPE, "%d optimizer groups: the grouped Adam step takes 1 to %d", n_groups,
                adam_groups::kMaxGroups);
    MLA_REQUIRE(mla::aligned(groups_dev, 16), MLA_E_ARG, "the group rows must be 16-byte aligned");
    GroupTable tab;
    for (int i = 0; i < n_groups; ++i) {
        const mla_adam_group_t& h = groups[i];
        const adam_groups::Scalars s = adam_groups::scalars(h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.decoupled != 0, h.amsgrad != 0, step);
        for (int k = 0; k < adam_groups::kGroupFloats; ++k) tab.v[i * adam_groups::kGroupFloats + k] = s.v[k];
    }
    for (int i = n_groups * adam_groups::kGroupFloats; i < adam_groups::kMaxGroups * adam_groups::kGroupFloats; ++i) tab.v[i] = 0.f;
    hipLaunchKernelGGL(set_groups_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), groups_dev, tab,
                       n_groups * adam_groups::kGroupFloats);
    MLA_LAUNCH_OK("adam_groups_prepare");
    return MLA_OK;
}

extern "C" int mla_adam_grouped_step(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, const int64_t* table_dev,
                                     int64_t table_words, int64_t n_runs, int64_t n_pads, const float* groups_dev, int n_groups,
                                     const float* coef_dev, mla_stream_t stream) {
    MLA_REQUIRE(p && g && m && v && table_dev && groups_dev && n >= 0 && n_runs >= 1 && n_pads >= 0, MLA_E_ARG, "bad grouped adam arguments");
    MLA_REQUIRE(n_groups >= 1 && n_groups <= adam_groups::kMaxGroups, MLA_E_SHAPE, "%d optimizer groups: the grouped Adam step takes 1 to %d",
                n_groups, adam_groups::kMaxGroups);
    MLA_REQUIRE(n % 4 == 0, MLA_E_SHAPE, "the flat buffers hold tensors padded to 4 floats: n = %lld is no multiple of 4", (long long)n);
    MLA_REQUIRE(mla::aligned(p, 16) && mla::aligned(g, 16) && mla::aligned(m, 16) && mla::aligned(v, 16) && mla::aligned(vmax, 16) &&
                mla::aligned(groups_dev, 16) && mla::aligned(table_dev, 8), MLA_E_ARG, "the flat buffers must be 16-byte aligned");
    if (n == 0) return MLA_OK;
    const int64_t chunks = adam_groups::chunks_of(n);
    MLA_REQUIRE(adam_groups::words_of(n_runs, chunks, n_pads) <= table_words, MLA_E_ARG, "the table is shorter than its sections: %lld words",
                (long long)table_words);
    hipLaunchKernelGGL(adam_grouped_kernel, dim3(unsigned(chunks < adam_groups::kAdamMaxGrid ? chunks : adam_groups::kAdamMaxGrid)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), p, g, m, v, vmax, n, table_dev, n_runs, chunks, n_pads, groups_dev, n_groups, coef_dev);
    MLA_LAUNCH_OK("adam (grouped)");
    return MLA_OK;
}

extern "C" int64_t mla_grad_norm_workspace_bytes(void) { return int64_t(adam_groups::kNormMaxGrid) * int64_t(sizeof(double)); }

extern "C" int mla_grad_norm(const float* g, int64_t n, float max_norm, void* workspace, float* norm_coef_dev, mla_stream_t stream) {
    MLA_REQUIRE(g && workspace && norm_coef_dev && n >= 1, MLA_E_ARG, "bad grad_norm arguments");
    MLA_REQUIRE(mla::aligned(g, 16) && mla::aligned(workspace, 8), MLA_E_ARG, "grad_norm: the gradient must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = int(adam_groups::norm_blocks(n));
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(unsigned(blocks)), dim3(256), 0, s, g, n, static_cast<double*>(workspace));
    MLA_LAUNCH_OK("grad_norm partial");
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, s, static_cast<const double*>(workspace), blocks, max_norm, norm_coef_dev);
    MLA_LAUNCH_OK("grad_norm finish");
    return MLA_OK;
}

extern "C" int mla_counter_add(int64_t* counter_dev, int64_t delta, mla_stream_t stream) {
    MLA_REQUIRE(counter_dev, MLA_E_ARG, "null counter");
    hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), counter_dev, delta);
    MLA_LAUNCH_OK("counter_add");
    return MLA_OK;
}

extern "C" int mla_dropout_mask_dev(uint8_t* mask, int64_t n, uint64_t seed, uint64_t stream_base, const int64_t* counter_dev,
                                    uint64_t offset, float p_drop, mla_stream_t stream) {
    MLA_REQUIRE(mask && counter_dev && n >= 0 && p_drop >= 0.f && p_drop <= 1.f, MLA_E_ARG, "bad dropout_mask arguments");
    if (n == 0) return MLA_OK;
    const uint32_t thresh = uint32_t(llround(double(p_drop) * double(1 << 24)));
    hipLaunchKernelGGL(dropout_mask_dev_kernel, dim3(grid_for((n + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), mask, n, seed,
                       stream_base, counter_dev, offset, thresh);
    MLA_LAUNCH_OK("dropout_mask (device stream count)");
    return MLA_OK;
}

extern "C" int mla_dropout_mask(uint8_t* mask, int64_t n, uint64_t seed, uint64_t stream_id, uint64_t offset, float p_drop,
                                mla_stream_t stream) {
    MLA_REQUIRE(mask && n >= 0 && p_drop >= 0.f && p_drop <= 1.f, MLA_E_ARG, "bad dropout_mask arguments");
    if (n == 0) return MLA_OK;
    const uint64_t key = mix64(seed * 0x9E3779B97F4A7C15ull + stream_id);
    const uint32_t thresh = uint32_t(llround(double(p_drop) * double(1 << 24)));
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for((n + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), mask, n, key,
                       offset, thresh);
    MLA_LAUNCH_OK("dropout_mask");
    return MLA_OK;
}
