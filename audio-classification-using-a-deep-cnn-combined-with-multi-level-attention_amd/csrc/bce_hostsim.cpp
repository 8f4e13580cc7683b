// bce_hostsim.cpp -- the two kernels of the binary cross-entropy (bce.hip) simulated on the host: the functions of bce_core.h,
// called lane by lane and thread by thread in the kernels' order (64 lanes striding over a row, xor butterflies over 32 ... 1,
// 256 threads striding over the rows, the LDS tree over 128 ... 1), in float32 with logf where the device has __logf. Every
// read of p and of the targets is recorded (the highest element index of each) and every store to dp counted per element.
// Built by tests/test_bce_cpu.py (g++ -shared); with -DBCE_HOSTSIM_MAIN a stand-alone program over a 5 x 65 case, for a sanitizer
// build of the host code.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bce_core.h"

namespace {

template <typename T>
T tree_256(std::vector<T>& part) {
    for (int o = 128; o > 0; o >>= 1)
        for (int t = 0; t < o; ++t) part[t] += part[t + o];
    return part[0];
}

template <typename T>
void butterfly_sum(T* v) {
    for (int o = 32; o > 0; o >>= 1) {
        T next[bce::kLanes];
        for (int l = 0; l < bce::kLanes; ++l) next[l] = v[l] + v[l ^ o];
        for (int l = 0; l < bce::kLanes; ++l) v[l] = next[l];
    }
}

}  // namespace

// 0, or -1 / -2 for what mla_bce refuses. max_read[0]: highest index read of p, [1]: of the targets.
extern "C" int hostsim_bce(const float* p, int64_t ldp, const float* y, int64_t ldt, int64_t rows, int K, const float* w, int reduction,
                           float scale, float* loss, float* dp, int64_t ld_dp, int32_t* writes, int32_t* counts, int64_t* max_read) {
    if (!p || !y || !loss || !counts || rows <= 0 || ldp < K || ldt < K || (dp && ld_dp < K)) return -1;
    if (K < 1 || K > bce::kMaxK) return -2;
    if (reduction != bce::kMean && reduction != bce::kSum) return -1;
    if (reduction == bce::kMean && !(scale > 0.f && scale <= 3.4028234e38f)) return -1;
    const float s = bce::scale_of(reduction, scale);
    max_read[0] = max_read[1] = -1;
    std::vector<double> term(rows);
    std::vector<int32_t> right(rows), bad(rows);
    for (int64_t b = 0; b < rows; ++b) {                                 // bce_rows_kernel: wave b
        float t[bce::kLanes];
        int nr[bce::kLanes], nb[bce::kLanes];
        for (int lane = 0; lane < bce::kLanes; ++lane) {
            float pv[bce::kPerLane], yv[bce::kPerLane], wv[bce::kPerLane];
            for (int j = 0; j < bce::kPerLane; ++j) {
                const int k = lane + bce::kLanes * j;
                pv[j] = yv[j] = 0.f;
                wv[j] = 1.f;
                if (k < K) {
                    pv[j] = p[b * ldp + k];
                    yv[j] = y[b * ldt + k];
                    if (w) wv[j] = w[k];
                    max_read[0] = std::max(max_read[0], b * ldp + k);
                    max_read[1] = std::max(max_read[1], b * ldt + k);
                }
            }
            t[lane] = 0.f;
            nr[lane] = nb[lane] = 0;
            for (int j = 0; j < bce::kPerLane; ++j) {
                const int k = lane + bce::kLanes * j;
                if (k < K) {
                    const bce::Cell c = bce::cell(pv[j], yv[j], wv[j], s, dp != nullptr);
                    t[lane] += c.term;
                    nr[lane] += c.right;
                    nb[lane] += c.bad;
                    if (dp) {
                        dp[b * ld_dp + k] = c.grad;
                        if (writes) writes[b * ld_dp + k] += 1;
                    }
                }
            }
        }
        butterfly_sum(t);
        butterfly_sum(nr);
        butterfly_sum(nb);
        term[b] = double(t[0]);
        right[b] = nr[0];
        bad[b] = nb[0];
    }
    std::vector<double> part(bce::kThreads);                             // bce_finish_kernel
    std::vector<int> ipart[3] = {std::vector<int>(bce::kThreads), std::vector<int>(bce::kThreads), std::vector<int>(bce::kThreads)};
    for (int tid = 0; tid < bce::kThreads; ++tid) {
        int n3[3];
        part[tid] = bce::finish_thread(term.data(), right.data(), bad.data(), rows, K, tid, n3);
        for (int i = 0; i < 3; ++i) ipart[i][tid] = n3[i];
    }
    const double sum = tree_256(part);
    for (int i = 0; i < 3; ++i) counts[i] = tree_256(ipart[i]);
    *loss = bce::finish_loss(sum, counts[1], s);
    return 0;
}

extern "C" int64_t hostsim_bce_workspace_bytes(int64_t rows) { return bce::workspace_bytes(rows); }

#ifdef BCE_HOSTSIM_MAIN
// 5 x 65 (one cell in the second stride of lane 0, one row in a second workgroup), weights; buffers sized exactly, so that a
// sanitizer sees any access past them.
int main() {
    const int64_t rows = 5, ldp = 67, ldt = 66;
    const int K = 65;
    std::vector<float> p((rows - 1) * ldp + K), y((rows - 1) * ldt + K), w(K), dp(rows * K);
    std::vector<int32_t> writes(rows * K, 0);
    for (size_t i = 0; i < p.size(); ++i) p[i] = 0.02f + 0.96f * float((i * 37) % 101) / 100.f;
    for (size_t i = 0; i < y.size(); ++i) y[i] = (i % 7 == 0) ? 0.3f : float((i * 13) % 3 == 0);
    for (int k = 0; k < K; ++k) w[k] = 0.25f + float(k % 16) * 0.25f;
    int wrong = 0;
    for (int reduction = 0; reduction < 2; ++reduction) {
        float loss = 0.f;
        int32_t counts[3];
        int64_t max_read[2];
        std::fill(writes.begin(), writes.end(), 0);
        const int rc = hostsim_bce(p.data(), ldp, y.data(), ldt, rows, K, w.data(), reduction, 1.f / float(rows * K), &loss, dp.data(), K,
                                   writes.data(), counts, max_read);
        for (int32_t n : writes) wrong += n != 1;
        wrong += rc != 0 || counts[1] != 0 || !(loss > 0.f) || max_read[0] != (rows - 1) * ldp + K - 1 || max_read[1] != (rows - 1) * ldt + K - 1;
        std::printf("reduction %d: rc %d loss %.6f counts %d %d %d max_read %lld %lld\n", reduction, rc, loss, counts[0], counts[1], counts[2],
                    (long long)max_read[0], (long long)max_read[1]);
    }
    std::printf(wrong ? "FAILED\n" : "ok\n");
    return wrong ? 1 : 0;
}
#endif
