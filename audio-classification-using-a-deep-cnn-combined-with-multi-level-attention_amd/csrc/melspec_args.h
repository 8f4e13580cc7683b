// melspec_args.h -- host-only argument checks of the mel-dB entries, shared by melspec.hip (forward) and melspec_bwd.hip (backward)
// so that both report one set of codes and mla_last_error texts.
#ifndef MLA_MELSPEC_ARGS_H
#define MLA_MELSPEC_ARGS_H

#include "common.h"
#include "melspec_core.h"

namespace melspec {

inline int check_signal(int64_t n_samples, int64_t hop, int64_t n_mels) {
    MLA_REQUIRE(hop >= 1, MLA_E_ARG, "melspec hop %lld < 1", (long long)hop);
    MLA_REQUIRE(n_mels >= 1 && n_mels <= kMaxMels, MLA_E_ARG, "melspec n_mels %lld outside [1, %d]", (long long)n_mels, kMaxMels);
    MLA_REQUIRE(n_samples >= kMinSamples, MLA_E_SHORT, "melspec needs at least %d samples per clip for reflect padding by %d (got %lld)",
                kMinSamples, kPad, (long long)n_samples);
    MLA_REQUIRE(n_samples <= (1 << 30), MLA_E_SHAPE, "melspec clips longer than 2^30 samples are not supported (got %lld)", (long long)n_samples);
    return MLA_OK;
}
inline int64_t runs_of(int64_t n_samples, int64_t hop) {
    const int64_t frames = 1 + n_samples / hop, per = run_frames(hop);
    return (frames + per - 1) / per;
}
inline int check_images(int64_t frames, float top_db, int64_t n_images, int64_t image_w, int64_t image_stride) {
    MLA_REQUIRE(top_db >= 0.f, MLA_E_ARG, "melspec top_db must be non-negative (got %g)", double(top_db));
    MLA_REQUIRE(n_images >= 1 && image_w >= 1 && image_stride >= 0, MLA_E_ARG, "bad melspec image arguments (%lld images of width %lld, stride %lld)",
                (long long)n_images, (long long)image_w, (long long)image_stride);
    MLA_REQUIRE(image_w <= frames && image_stride <= frames && (n_images - 1) * image_stride + image_w <= frames, MLA_E_SHAPE,
                "images leave the %lld-column spectrogram (%lld images of width %lld, stride %lld)", (long long)frames, (long long)n_images,
                (long long)image_w, (long long)image_stride);
    return MLA_OK;
}

}  // namespace melspec
#endif
