// melspec_tables.h -- host-side construction of the mel-dB kernel's constant tables in double precision, rounded
// once to float: the periodic Hann window (scipy.signal.get_window("hann", 2048, fftbins=True)), the FFT twiddles,
// and librosa.filters.mel(sr, 2048, n_mels, fmin, fmax, htk, norm="slaney") in sparse form (per band: first bin, bin
// count, offset into the packed weights). MelConfig names the basis; the (sr, n_mels) overloads are librosa's defaults
// (fmin 0, fmax sr / 2, Slaney scale), the ResNet branch's. Shared by melspec.hip (mla_melspec_build_tables,
// mla_melspec_build_band_tables) and the host simulations used by the CPU tests.
#ifndef MLA_MELSPEC_TABLES_H
#define MLA_MELSPEC_TABLES_H

#include <cmath>
#include <cstring>
#include <vector>

#include "melspec_core.h"

namespace melspec {

constexpr double kFsp = 200.0 / 3.0, kMinLogHz = 1000.0, kMinLogMel = kMinLogHz / kFsp;
inline double logstep() { return std::log(6.4) / 27.0; }

inline double hz_to_mel(double hz) { return hz >= kMinLogHz ? kMinLogMel + std::log(hz / kMinLogHz) / logstep() : hz / kFsp; }
inline double mel_to_hz(double mel) { return mel >= kMinLogMel ? kMinLogHz * std::exp(logstep() * (mel - kMinLogMel)) : kFsp * mel; }
// the HTK scale (librosa's htk=True): mel = 2595 log10(1 + hz / 700)
inline double hz_to_mel_htk(double hz) { return 2595.0 * std::log10(1.0 + hz / 700.0); }
inline double mel_to_hz_htk(double mel) { return 700.0 * (std::pow(10.0, mel / 2595.0) - 1.0); }

struct MelConfig {
    double sr;
    int64_t n_mels;
    double fmin, fmax;
    bool htk;
};
inline MelConfig default_config(double sr, int64_t n_mels) { return MelConfig{sr, n_mels, 0.0, sr / 2.0, false}; }

// numpy.linspace(lo, hi, count)[i]
inline double linspace(double lo, double hi, int count, int i) { return i == count - 1 ? hi : lo + i * ((hi - lo) / (count - 1)); }

// dense row b of the (n_mels, 1025) Slaney-normalised filterbank
inline void mel_row(const MelConfig& c, int b, double* row) {
    const double sr = c.sr;
    const double lo = c.htk ? hz_to_mel_htk(c.fmin) : hz_to_mel(c.fmin), hi = c.htk ? hz_to_mel_htk(c.fmax) : hz_to_mel(c.fmax);
    double f[3];
    for (int j = 0; j < 3; ++j) {
        const double mel = linspace(lo, hi, int(c.n_mels) + 2, b + j);
        f[j] = c.htk ? mel_to_hz_htk(mel) : mel_to_hz(mel);
    }
    const double enorm = 2.0 / (f[2] - f[0]);
    for (int k = 0; k < kBins; ++k) {
        const double hz = linspace(0.0, sr / 2.0, kBins, k);
        const double lower = (hz - f[0]) / (f[1] - f[0]), upper = (f[2] - hz) / (f[2] - f[1]);
        const double w = lower < upper ? lower : upper;
        row[k] = w > 0.0 ? w * enorm : 0.0;
    }
}

struct Band { int first, bins; };

inline Band band_support(const double* row) {
    int k0 = -1, k1 = -1;
    for (int k = 0; k < kBins; ++k)
        if (row[k] != 0.0) { if (k0 < 0) k0 = k; k1 = k; }
    return k0 < 0 ? Band{0, 0} : Band{k0, k1 - k0 + 1};
}

inline bool valid_config(double sr, int64_t n_mels) { return sr > 0.0 && std::isfinite(sr) && n_mels >= 1 && n_mels <= kMaxMels; }
// a band edge outside 0 <= fmin < fmax <= sr / 2 has no meaning on the 1025 bin centres
inline bool valid_config(const MelConfig& c) {
    return valid_config(c.sr, c.n_mels) && c.fmin >= 0.0 && c.fmin < c.fmax && c.fmax <= c.sr / 2.0;
}

// floats of the whole table; -1 for an invalid configuration
inline int64_t table_floats(const MelConfig& c) {
    if (!valid_config(c)) return -1;
    std::vector<double> row(kBins);
    int64_t nnz = 0;
    for (int b = 0; b < c.n_mels; ++b) { mel_row(c, b, row.data()); nnz += band_support(row.data()).bins; }
    return tab_weights(int(c.n_mels)) + nnz;
}
inline int64_t table_floats(double sr, int64_t n_mels) { return valid_config(sr, n_mels) ? table_floats(default_config(sr, n_mels)) : -1; }

inline int build_tables(const MelConfig& c, float* tab) {
    if (!valid_config(c)) return -1;
    const int64_t n_mels = c.n_mels;
    const double pi = 3.14159265358979323846;
    for (int n = 0; n < kFft; ++n) tab[kTabWindow + n] = float(0.5 - 0.5 * std::cos(2.0 * pi * n / kFft));
    for (int k = 0; k < kTw; ++k) {
        tab[kTabTw + 2 * k] = float(std::cos(2.0 * pi * k / kFft));
        tab[kTabTw + 2 * k + 1] = float(-std::sin(2.0 * pi * k / kFft));
    }
    int* meta = reinterpret_cast<int*>(tab + kTabMeta);
    float* weights = tab + tab_weights(int(n_mels));
    std::vector<double> row(kBins);
    int offset = 0;
    for (int b = 0; b < n_mels; ++b) {
        mel_row(c, b, row.data());
        const Band s = band_support(row.data());
        meta[3 * b] = s.first; meta[3 * b + 1] = s.bins; meta[3 * b + 2] = offset;
        for (int i = 0; i < s.bins; ++i) weights[offset + i] = float(row[s.first + i]);   // zeros inside the support stay zero weights
        offset += s.bins;
    }
    return 0;
}
inline int build_tables(double sr, int64_t n_mels, float* tab) { return valid_config(sr, n_mels) ? build_tables(default_config(sr, n_mels), tab) : -1; }

}  // namespace melspec
#endif
