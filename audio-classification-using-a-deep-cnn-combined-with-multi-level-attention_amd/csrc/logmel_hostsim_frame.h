// logmel_hostsim_frame.h -- TEST HARNESS (never part of libmla_hip.so, included by no .hip file): one STFT frame on the host
// through logmel_core.h's per-lane phases, the 16 lanes of a group one after the other, with a plain array standing in for the
// group's LDS exchange buffer. Shared by logmel_hostsim.cpp, logmel_bags_hostsim.cpp and logmel_timeline_hostsim.cpp.
#ifndef MLA_LOGMEL_HOSTSIM_FRAME_H
#define MLA_LOGMEL_HOSTSIM_FRAME_H

#include "logmel_core.h"
#include "logmel_tables.h"

namespace logmel {

// one STFT frame -> 64 log-mel bands; c[j] = lane j's constants of the tables `tab`
inline void frame_row(const LaneConsts* c, const float* tab, const float* frame, float* row) {
    float xch[2 * 16 * kXchStride];
    float re[16][16], im[16][16], vr[16][8], vi[16][8];
    for (int j = 0; j < 16; ++j) phase1(c[j], j, frame, tab + kTabWindow, xch);
    for (int j = 0; j < 16; ++j) phase2_read(j, xch, re[j], im[j]);
    for (int j = 0; j < 16; ++j) phase2_fft(re[j], im[j]);
    for (int j = 0; j < 16; ++j) phase3_view(j, re[j], im[j], vr[j], vi[j]);
    float* mag = xch;                                          // magnitudes alias the dead exchange buffer
    for (int j = 0; j < 16; ++j) {                             // the 16-lane exchange: partner = (16 - j) & 15
        const int partner = (16 - j) & 15;
        phase3_pairs(j, re[j], im[j], vr[partner], vi[partner], mag, tab + kTabPw + kPwRow * j);
    }
    for (int j = 0; j < 16; ++j) {
        float o[4];
        phase4(c[j], j, mag, tab + kTabMelW + kMelRow * j, o);
        for (int s = 0; s < 4; ++s) row[band_of(j, s)] = o[s];
    }
}

}  // namespace logmel

#endif
