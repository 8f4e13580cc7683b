// adam_groups.h -- host-only logic of the grouped Adam step (train_kernels.hip): the table that tells the kernel which
// optimizer group owns which stretch of the flat parameter buffer, and the per-group scalars of one step. Plain C++ (no HIP
// types), so that the table can be built and checked without a device (mla_adam_groups_table).
//
// The flat buffer holds the tensors in named_parameters() order, each padded to a multiple of 4 floats (16-byte starts). A RUN
// is a maximal stretch of adjacent tensors of one group in those padded coordinates. The kernel works in CHUNKS of kAdamChunk
// elements; per chunk the table gives the run that holds the chunk's first element (the kernel walks on from there, a quad of
// four elements never straddles a run) and the range of PAD entries inside the chunk: the quads that end a tensor whose size is
// no multiple of 4, with the count of real elements in them -- the rest of such a quad is padding and is left exactly as it is.
//
// Layout of the table, int64 words:  run_end[R] | run_group[R] | chunk_run[C] | chunk_pad[C + 1] | (pad_quad, pad_valid)[P]
#ifndef MLA_ADAM_GROUPS_H
#define MLA_ADAM_GROUPS_H

#include <cmath>
#include <cstdint>

namespace adam_groups {

constexpr int kMaxGroups = 64;               // per-group scalars travel as ONE kernel argument (64 * 8 floats = 2 KiB of the 4 KiB limit)
constexpr int kGroupFloats = 8;              // device row of one group: see Scalars below
constexpr int kAdamChunk = 2048;             // elements per workgroup iteration: 256 lanes x 2 quads of 4 floats
constexpr int kAdamMaxGrid = 2048;           // workgroups at most (8 per CU on 256 CUs); one sweep = 2048 * 2048 = 4 194 304 elements
constexpr int kNormChunk = 4096;             // elements per workgroup iteration of the norm pass
constexpr int kNormMaxGrid = 1024;           // = partial sums the finishing block adds (workspace: 1024 doubles)

enum Flags { kL2 = 1, kDecoupled = 2, kAmsgrad = 4 };

inline int64_t pad4(int64_t k) { return (k + 3) / 4 * 4; }
inline int64_t chunks_of(int64_t n) { return (n + kAdamChunk - 1) / kAdamChunk; }

struct Counts { int64_t total, runs, pads, chunks, words; };

inline int64_t words_of(int64_t runs, int64_t chunks, int64_t pads) { return 2 * runs + chunks + (chunks + 1) + 2 * pads; }

// 0 or which argument is wrong: 1 = a tensor without elements, 2 = a group index outside [0, n_groups), 3 = n_groups outside [1, 64]
inline int count(const int64_t* numel, const int32_t* group, int64_t n_tensors, int n_groups, Counts* c) {
    if (n_groups < 1 || n_groups > kMaxGroups) return 3;
    int64_t off = 0, runs = 0, pads = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        if (numel[i] <= 0) return 1;
        if (group[i] < 0 || group[i] >= n_groups) return 2;
        if (i == 0 || group[i] != group[i - 1]) ++runs;
        if (numel[i] % 4) ++pads;
        off += pad4(numel[i]);
    }
    c->total = off; c->runs = runs; c->pads = pads; c->chunks = chunks_of(off);
    c->words = words_of(runs, c->chunks, pads);
    return 0;
}

// fills `out` (c.words int64 words); count() has accepted the same arguments
inline void build(const int64_t* numel, const int32_t* group, int64_t n_tensors, const Counts& c, int64_t* out) {
    int64_t* run_end = out;
    int64_t* run_group = run_end + c.runs;
    int64_t* chunk_run = run_group + c.runs;
    int64_t* chunk_pad = chunk_run + c.chunks;
    int64_t* pad = chunk_pad + c.chunks + 1;
    int64_t off = 0, r = -1, p = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        if (i == 0 || group[i] != group[i - 1]) { ++r; run_group[r] = group[i]; }
        if (numel[i] % 4) { pad[2 * p] = off + numel[i] / 4 * 4; pad[2 * p + 1] = numel[i] % 4; ++p; }
        off += pad4(numel[i]);
        run_end[r] = off;
    }
    r = 0; p = 0;
    for (int64_t k = 0; k < c.chunks; ++k) {
        const int64_t start = k * kAdamChunk;
        while (run_end[r] <= start) ++r;
        chunk_run[k] = r;
        while (p < c.pads && pad[2 * p] < start) ++p;
        chunk_pad[k] = p;
    }
    chunk_pad[c.chunks] = c.pads;
}

// The device row of one group at step t. Computed in double exactly as mla_adam_step / mla_adam_prepare compute their pair, so a
// single group without options gives the old kernel's bits.
struct Scalars { float v[kGroupFloats]; };   // step_size, 1/sqrt(bc2), beta1, beta2, eps, decay, flags (a small integer), 0

inline Scalars scalars(float lr, float beta1, float beta2, float eps, float weight_decay, bool decoupled, bool amsgrad, int64_t step) {
    const double bc1 = 1.0 - std::pow(double(beta1), double(step)), bc2 = 1.0 - std::pow(double(beta2), double(step));
    int flags = amsgrad ? kAmsgrad : 0;
    float decay = 0.f;
    if (weight_decay != 0.f) {
        flags |= decoupled ? kDecoupled : kL2;
        // torch: param.mul_(1 - lr * weight_decay) (decoupled) | grad.add(param, alpha=weight_decay) (L2)
        decay = decoupled ? float(1.0 - double(lr) * double(weight_decay)) : weight_decay;
    }
    Scalars s;
    s.v[0] = float(double(lr) / bc1);
    s.v[1] = float(1.0 / std::sqrt(bc2));
    s.v[2] = beta1; s.v[3] = beta2; s.v[4] = eps; s.v[5] = decay;
    s.v[6] = float(flags);
    s.v[7] = 0.f;
    return s;
}

inline int64_t norm_blocks(int64_t n) {      // depends on n only: the summation order is a function of the size
    const int64_t b = (n + kNormChunk - 1) / kNormChunk;
    return b < 1 ? 1 : (b > kNormMaxGrid ? kNormMaxGrid : b);
}

}  // namespace adam_groups

#endif
