// ce_hostsim.cpp -- the three kernels of the cross-entropy with options (train_kernels.hip) simulated on the host: the functions of
// ce_core.h, called lane by lane and thread by thread in the kernels' order (64 lanes striding over a row, xor butterflies over
// 32 ... 1, 256 threads striding over the rows, the LDS tree over 128 ... 1), in float32 with expf / logf where the device has
// __expf / __logf. Every read of x is recorded (the highest element index) and every store to dx counted per element.
// Built by tests/test_ce_opts_cpu.py (g++ -shared); with -DCE_HOSTSIM_MAIN a stand-alone program over a 3 x 65 case, for a
// sanitizer build of the host code.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ce_core.h"

namespace {

template <typename T>
T tree_256(std::vector<T>& part) {
    for (int o = 128; o > 0; o >>= 1)
        for (int t = 0; t < o; ++t) part[t] += part[t + o];
    return part[0];
}

template <typename T, typename Op>
void butterfly(T* v, Op op) {
    for (int o = 32; o > 0; o >>= 1) {
        T next[ce::kLanes];
        for (int l = 0; l < ce::kLanes; ++l) next[l] = op(v[l], v[l ^ o]);
        for (int l = 0; l < ce::kLanes; ++l) v[l] = next[l];
    }
}

float add(float a, float b) { return a + b; }

}  // namespace

// 0, or -1 / -2 for what mla_cross_entropy_opts refuses. den_out[0]: the simulated mla_cross_entropy_den (mean only).
extern "C" int hostsim_ce_opts(const float* x, int64_t ldx, const int64_t* labels, int64_t rows, int K, const float* w, int64_t ignore_index,
                               float smoothing, int reduction, float* den_out, float* loss, float* dx, int64_t ld_dx, int32_t* writes,
                               int32_t* counts, int64_t* max_read) {
    if (!x || !labels || !loss || !counts || rows <= 0 || ldx < K || (dx && ld_dx < K)) return -1;
    if (K < 1 || K > ce::kMaxK) return -2;
    if (!(smoothing >= 0.f && smoothing <= 1.f) || (reduction != ce::kMean && reduction != ce::kSum)) return -1;
    *max_read = -1;
    float den = 0.f;
    if (reduction == ce::kMean) {                                        // cross_entropy_den_kernel
        std::vector<double> part(ce::kThreads);
        for (int t = 0; t < ce::kThreads; ++t) part[t] = ce::den_thread(labels, rows, K, w, ignore_index, t);
        den = float(tree_256(part));
        if (den_out) *den_out = den;
    }
    const float* scale = reduction == ce::kMean ? &den : nullptr;
    std::vector<double> term(rows);
    std::vector<int32_t> flags(rows);
    auto store = [&](int64_t b, int k, float v) {
        dx[b * ld_dx + k] = v;
        if (writes) writes[b * ld_dx + k] += 1;
    };
    for (int64_t b = 0; b < rows; ++b) {                                 // cross_entropy_opts_kernel: wave b
        const int64_t y64 = labels[b];
        const int cls = ce::classify(y64, K, ignore_index);
        if (cls != ce::kCounted) {
            if (dx)
                for (int lane = 0; lane < ce::kLanes; ++lane)
                    for (int k = lane; k < K; k += ce::kLanes) store(b, k, 0.f);
            term[b] = 0.0;
            flags[b] = cls;
            continue;
        }
        float xv[ce::kLanes][ce::kPerLane];
        for (int lane = 0; lane < ce::kLanes; ++lane)
            for (int j = 0; j < ce::kPerLane; ++j) {
                const int k = lane + ce::kLanes * j;
                xv[lane][j] = 0.f;
                if (k < K) {
                    xv[lane][j] = x[b * ldx + k];
                    if (b * ldx + k > *max_read) *max_read = b * ldx + k;
                }
            }
        ce::MaxAt top[ce::kLanes];
        for (int lane = 0; lane < ce::kLanes; ++lane) top[lane] = ce::lane_max(xv[lane], K, lane);
        butterfly(top, ce::max_combine);
        float se[ce::kLanes];
        for (int lane = 0; lane < ce::kLanes; ++lane) se[lane] = ce::lane_sum_exp(xv[lane], K, lane, top[lane].m);
        butterfly(se, add);
        ce::Row r;
        r.y = int(y64);
        r.lse = top[0].m + ce::fast_log(se[0]);
        r.c = (1.f - smoothing) * (w ? w[r.y] : 1.f);
        r.ek = smoothing / float(K);
        r.wsum = 0.f;
        r.s = scale ? 1.f / scale[0] : 1.f;
        float t = 0.f;
        if (r.ek > 0.f) {
            float tl[ce::kLanes], wl[ce::kLanes];
            for (int lane = 0; lane < ce::kLanes; ++lane) ce::lane_smooth(xv[lane], w, K, lane, r.lse, &tl[lane], &wl[lane]);
            butterfly(tl, add);
            butterfly(wl, add);
            t = tl[0];
            r.wsum = wl[0];
        }
        if (dx)
            for (int lane = 0; lane < ce::kLanes; ++lane)
                for (int j = 0; j < ce::kPerLane; ++j) {
                    const int k = lane + ce::kLanes * j;
                    if (k < K) store(b, k, ce::dx_elem(r, xv[lane][j], k, (w && r.ek > 0.f) ? w[k] : 1.f));
                }
        term[b] = ce::row_loss(r, x[b * ldx + r.y], t);
        flags[b] = ce::kCounted | (top[0].i == r.y ? ce::kHit : 0);
    }
    std::vector<double> part(ce::kThreads);                              // cross_entropy_finish_kernel
    std::vector<int> ipart[3] = {std::vector<int>(ce::kThreads), std::vector<int>(ce::kThreads), std::vector<int>(ce::kThreads)};
    for (int t = 0; t < ce::kThreads; ++t) {
        int n3[3];
        part[t] = ce::finish_thread(term.data(), flags.data(), rows, t, n3);
        for (int i = 0; i < 3; ++i) ipart[i][t] = n3[i];
    }
    const double sum = tree_256(part);
    for (int i = 0; i < 3; ++i) counts[i] = tree_256(ipart[i]);
    *loss = ce::finish_loss(sum, counts[1], reduction, scale);
    return 0;
}

extern "C" int64_t hostsim_ce_workspace_bytes(int64_t rows) { return ce::workspace_bytes(rows); }

#ifdef CE_HOSTSIM_MAIN
// 3 x 65 (one element in the second stride of lane 0), weights, smoothing, one ignored row; buffers sized exactly, so that a
// sanitizer sees any access past them.
int main() {
    const int64_t rows = 3, ldx = 67;
    const int K = 65;
    std::vector<float> x(rows * ldx), w(K), dx(rows * K);
    std::vector<int64_t> labels = {64, -100, 7};
    std::vector<int32_t> writes(rows * K, 0);
    for (size_t i = 0; i < x.size(); ++i) x[i] = float(int((i * 37) % 101) - 50) * 0.08f;
    for (int k = 0; k < K; ++k) w[k] = 0.25f + float(k % 16) * 0.25f;
    int bad = 0;
    for (int reduction = 0; reduction < 2; ++reduction) {
        float den = 0.f, loss = 0.f;
        int32_t counts[3];
        int64_t max_read = 0;
        std::fill(writes.begin(), writes.end(), 0);
        const int rc = hostsim_ce_opts(x.data(), ldx, labels.data(), rows, K, w.data(), -100, 0.1f, reduction, &den, &loss, dx.data(), K,
                                       writes.data(), counts, &max_read);
        for (int32_t n : writes) bad += n != 1;
        bad += rc != 0 || counts[2] != 2 || counts[1] != 0 || !(loss > 0.f) || max_read != (rows - 1) * ldx + K - 1;
        std::printf("reduction %d: rc %d loss %.6f den %.4f counts %d %d %d max_read %lld\n", reduction, rc, loss, den, counts[0], counts[1],
                    counts[2], (long long)max_read);
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
