/*
 * mla_hip.h -- C ABI of libmla_hip.so: the MI355X (gfx950) hot path of
 * caesar-one/audio-classification-using-a-deep-cnn-combined-with-multi-level-attention
 *
 *   waveform -> framed STFT -> mel -> log -> VGGish conv stack -> FC embeddings
 *            -> multi-level attention pooling -> class scores  (+ the training step)
 *
 * The reference has no FFI: its callers use Python functions / nn.Module classes
 * directly. Each entry point below names the reference
 * interface (file:line under the reference tree) whose arithmetic it replaces; the
 * Python drop-in modules in the package bind them with ctypes.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers (unless a parameter says "host"), explicit int64
 *     sizes, a hipStream_t passed as void*, caller-provided workspaces;
 *   - every function returns 0 on success or a negative MLA_E_* code; the message is
 *     available from mla_last_error() (thread-local);
 *   - no allocation, no host synchronisation and no implicit stream inside: kernels are
 *     enqueued on the given stream and the caller keeps the buffers alive until they
 *     have run (graph-capturable);
 *   - shapes are checked on the host BEFORE any launch; a shape the kernels were not
 *     compiled for is an error, never a silent fallback.
 */
#ifndef MLA_HIP_H
#define MLA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLA_OK            0
#define MLA_E_ARG        -1   /* null pointer / negative size / misaligned buffer        */
#define MLA_E_SHAPE      -2   /* shape not supported by the compiled kernels             */
#define MLA_E_SHORT      -3   /* waveform shorter than 240 samples (reference: ValueError,
                                 mel_features.py:42-45 via vggish_input.py:56)           */
#define MLA_E_LAUNCH     -4   /* hipLaunch / HIP runtime error                           */
#define MLA_E_DTYPE      -5   /* unknown dtype code                                      */

/* element types of activations / weights */
#define MLA_F32   0
#define MLA_BF16  1
#define MLA_I16   2
#define MLA_F64   4  /* mla_allreduce_flat (the BatchNorm sums travel in double precision); sample format of mla_clips_prepare_raw */
#define MLA_I32   5  /* mla_allreduce_flat (n_correct); sample format of mla_clips_prepare_raw                                    */
#define MLA_U8    6  /* unsigned 8-bit PCM: sample format of mla_clips_prepare_raw only                                          */
#define MLA_I24   7  /* signed 24-bit PCM, three packed little-endian bytes: sample format of mla_clips_prepare_raw only         */
#define MLA_BF16X3 3  /* "split" bf16: x = hi + lo, two bf16 planes [hi(C) | lo(C)] per row / pixel; three bf16 MFMA
                        * products per term (hi*hi + hi*lo + lo*hi) with f32 accumulation: f32-grade results (2^-18
                        * relative per product) at a third of the bf16 rate. Accepted by mla_vggish_conv1 (output),
                        * mla_vggish_conv and mla_linear_bf16x3; weights are prepared by mla_split_bf16x3. */

typedef void* mla_stream_t;            /* hipStream_t */

int         mla_abi_version(void);
const char* mla_last_error(void);

/* ------------------------------------------------------------------------------------
 * Front-end: torchvggish/mel_features.py + torchvggish/vggish_input.py
 * ---------------------------------------------------------------------------------- */

/* mel_features.py:42 and vggish_input.py:67-76 -- exact integer frame arithmetic for a
 * 16 kHz waveform: stft_frames = 1 + floor((n-400)/160), examples = 1 + floor((F-96)/96)
 * clamped at 0. Returns MLA_E_SHORT when the reference would raise (n < 240). Host only. */
int mla_logmel_counts(int64_t n_samples, int64_t* stft_frames, int64_t* examples);

/* Constant tables of the fused kernel (periodic Hann mel_features.py:48-68, HTK mel
 * matrix mel_features.py:114-189 in sparse per-lane form, FFT twiddles), computed in
 * double precision on the host. `host_out` receives mla_logmel_table_floats() floats;
 * the caller uploads them once and passes the device copy to mla_logmel_examples. */
int64_t mla_logmel_table_floats(void);
int     mla_logmel_build_tables(float* host_out);
/* Dense (257 x 64) double-precision mel matrix and 400-point window exactly as the
 * tables encode them (host; used by the CPU tests to pin the tables to the oracle). */
int     mla_logmel_reference_tables(double* host_window400, double* host_mel_257x64);

/* vggish_input.waveform_to_examples (vggish_input.py:30-82) for 16 kHz mono input:
 * pcm[n_wave][wave_stride] (first n_samples of each row used) -> examples
 * out[n_wave * examples][96][64], waveform-major, where examples comes from
 * mla_logmel_counts(n_samples). pcm_dtype: MLA_F32 (samples in [-1,1)) or MLA_I16
 * (scaled by 1/32768 as vggish_input.py:98 does). out_dtype: MLA_F32 or MLA_BF16.
 * One fused kernel: frame (mel_features.py:21-45) -> Hann -> |rfft 512|
 * (mel_features.py:71-92) -> mel (mel_features.py:220) -> log(. + 0.01) (:223) ->
 * 96-frame examples (vggish_input.py:73-76). */
int mla_logmel_examples(const void* pcm, int pcm_dtype, int64_t n_wave, int64_t n_samples,
                        int64_t wave_stride, const float* tables, void* out, int out_dtype,
                        mla_stream_t stream);

/* Gradient of mla_logmel_examples (MLA_F32 output) with respect to the WAVEFORM: the adjoint of frame -> Hann -> |rfft 512|
 * (mel_features.py:71-92) -> mel -> log(. + 0.01) (mel_features.py:220-223) -> 96-frame examples (vggish_input.py:56-76).
 * pcm / pcm_dtype / n_wave / n_samples / wave_stride / tables as for mla_logmel_examples (for MLA_I16 the gradient is with respect
 * to the float value pcm / 32768); bwd_tables: device copy of the mla_logmel_bwd_table_floats() floats mla_logmel_bwd_build_tables
 * writes (the transposed mel step, bin -> its <= 2 bands, and the split twiddles; built in double precision on the host from the
 * same mel matrix); d_examples (n_wave * examples, 96, 64) f32 = dL / d out; d_wave[n_wave][d_wave_stride] f32 = dL / d pcm.
 * The frames' spectra are recomputed. One launch, no workspace, no atomics: every d_wave[w][s], s < n_samples, is stored exactly
 * once (the caller zeroes nothing), a sample's <= 3 frames are summed in ascending frame order, samples from
 * 160 (96 examples - 1) + 400 on get exactly 0, and a row's bits depend neither on n_wave nor on the strides. |X_k| = 0 passes no
 * gradient (torch's sgn(0) = 0), never NaN or Inf. Conditioning: X_k / |X_k| is only meaningful in float32 where |X_k| is well
 * above the frame's rounding noise; on signals with bins far below their peak (a pure tone) ANY float32 evaluation is far from the
 * float64 gradient. That belongs to the function, not to this kernel.
 * Errors, all before any launch: null pointer, negative size, stride < n_samples -> MLA_E_ARG; n_samples < 240 -> MLA_E_SHORT;
 * pcm_dtype -> MLA_E_DTYPE. n_wave == 0 returns MLA_OK and touches nothing; examples == 0 writes zeros (d_examples may be null). */
int64_t mla_logmel_bwd_table_floats(void);
int     mla_logmel_bwd_build_tables(float* host_out);
int mla_logmel_examples_bwd(const void* pcm, int pcm_dtype, int64_t n_wave, int64_t n_samples, int64_t wave_stride,
                            const float* tables, const float* bwd_tables, const float* d_examples, float* d_wave,
                            int64_t d_wave_stride, mla_stream_t stream);

/* Stand-alone stages for ARBITRARY configurations of the reference API (any window / hop /
 * power-of-two fft_length <= 4096, any mel layout); the VGGish configuration on the hot path
 * uses mla_logmel_examples instead.
 * mla_stft_magnitude: mel_features.stft_magnitude (mel_features.py:71-92) of one 1-D f32 signal;
 *   window: window_length floats (host-built periodic Hann); twiddle: fft_length/2 pairs
 *   (cos, -sin)(2 pi m / fft_length); out: frames x (fft_length/2 + 1) magnitudes,
 *   frames = 1 + floor((n_samples - window_length) / hop_length) (none if the signal is shorter).
 * mla_mel_log: log(spectrogram . mel_matrix + log_offset) (mel_features.py:220-223);
 *   spectrogram frames x bins, mel_matrix bins x bands (row-major), out frames x bands. */
int mla_stft_magnitude(const float* signal, int64_t n_samples, const float* window, const float* twiddle,
                       int64_t window_length, int64_t hop_length, int64_t fft_length, float* out,
                       mla_stream_t stream);
int mla_mel_log(const float* spectrogram, const float* mel_matrix, int64_t frames, int64_t bins, int64_t bands,
                float log_offset, float* out, mla_stream_t stream);

/* Mono mix of waveform_to_examples (vggish_input.py:49-50, `np.mean(data, axis=1)`), with wavfile_to_examples' int16
 * scaling (vggish_input.py:98) when the input is MLA_I16: interleaved (n_samples, channels) PCM -> (n_samples) float32.
 * The mean is taken in double precision like numpy's on the reference's float64 data, then rounded once. */
int mla_mono_mix(const void* pcm, int pcm_dtype, int64_t n_samples, int channels, float* out, mla_stream_t stream);
/* dataset.create_spec (native path, dataset.py:318-324) + split (dataset.py:329-363): the caller of
 * waveform_to_examples in the reference's data pipeline. examples (clips*ex_per_clip, 96, 64) ->
 * out (clips, n_frames, 64, frame_len) with out[c][t][band][x] = spec_c[band][t*stride + x], where
 * spec_c is the (64, 384) concatenation of the clip's <= 4 transposed examples, zero-padded. */
int mla_dataset_frames(const float* examples, int64_t clips, int ex_per_clip, int n_frames, int frame_len,
                       int stride, float* out, mla_stream_t stream);
/* dataset.create_spec (native path, dataset.py:318-324) + split (dataset.py:329-363) for a RAGGED batch, log-mel included: one
 * launch from rows of 16 kHz mono PCM to the bag tensor load_hdf5(cnn_type="vggish", use_librosa=False) stores.
 * pcm[clips][row_stride] (MLA_F32, or MLA_I16 scaled by 1/32768; the first n_samples of a row are valid input); counts[clips]
 * (DEVICE, int32) says how many whole 0.96 s examples row c holds, 0..4; host_counts is the same array on the HOST, read for
 * validation before anything is launched. (n_frames, stride) is (10, 32) (overlapping_split) or (4, 96) (contiguous_split).
 * out[clips][n_frames][64][96], MLA_F32 or MLA_BF16 (one rounding of the f32 value), 16-byte aligned:
 *   out[c][t][b][x] = spec_c[b][t * stride + x],  spec_c[b][96 s + f] = log-mel of band b, frame f of example s for s < counts[c],
 * exactly 0.0 for s >= counts[c] (the reference pads missing slots of the spectrogram with 0.0, not ln 0.01) -- the bits
 * mla_logmel_examples + mla_dataset_frames give for the same samples. Every element of out is written exactly once; no spectrum
 * is computed for an absent slot and no sample beyond 15 600 + 15 360 (counts[c] - 1) of a row is read.
 * Errors, all before any launch: null pointer, count outside 0..4 -> MLA_E_ARG; a count whose samples exceed n_samples, another
 * (n_frames, stride) -> MLA_E_SHAPE; dtype codes -> MLA_E_DTYPE. clips == 0 returns MLA_OK and touches nothing. */
int mla_logmel_bags(const void* pcm, int pcm_dtype, int64_t clips, int64_t n_samples, int64_t row_stride, const int32_t* counts,
                    const int32_t* host_counts, int n_frames, int stride, const float* tables, void* out, int out_dtype,
                    mla_stream_t stream);
/* ---- Timelines: a recording of any length scored in windows of four examples at a hop of hop_slots * 0.32 s ----
 * Host only, the single source of the arithmetic. A 16 kHz recording of n_samples has log-mel columns 0 .. (n - 400) / 160; slot u
 * is columns [32 u, 32 u + 96). With q = hop_slots >= 1:
 *   n >= 61 680: windows = 1 + (n - 61 680) / (5 120 q); window j is the bag mla_logmel_bags gives for the crop
 *     [5 120 q j, 5 120 q j + 61 680), i.e. slots q j .. q j + 9; a trailing stretch that fills no window is dropped;
 *   240 <= n < 61 680: one window, the bag mla_logmel_bags gives (examples the recording lacks are 0.0).
 * A slot is kept iff u mod q < 10 (and u <= q (windows - 1) + 9); *slots is their number: q (windows - 1) + 10 for q <= 10, where
 * window j is rows q j .. q j + 9 of the recording's kept slots, and 10 * windows for q > 10, window j = rows 10 j .. 10 j + 9.
 * *samples_read = all a row must hold: 61 680 + 5 120 q (windows - 1), or 15 600 + 15 360 (examples - 1) (0 without an example).
 * Any output pointer may be NULL. n_samples < 240 -> MLA_E_SHORT (the reference raises); n_samples < 0 or hop_slots < 1 -> MLA_E_ARG. */
int mla_timeline_counts(int64_t n_samples, int64_t hop_slots, int64_t* windows, int64_t* slots, int64_t* samples_read);
/* The kept slots of a RAGGED batch of recordings in one launch, each column's spectrum computed once however many windows share it.
 * pcm[recordings][row_stride] as in mla_logmel_bags (the first n_samples of a row are valid input). desc[recordings][5] (DEVICE,
 * int64) and host_desc, the same array on the HOST, read for validation before anything is launched. Per recording:
 *   [0] first_slot  first row of out it writes: the kept slots of the recordings before it
 *   [1] cols        columns in its track: 32 q (windows - 1) + 384
 *   [2] spec_cols   columns that have a spectrum: cols, or for a one-window track 96 * examples (0, 96, 192 or 288)
 *   [3] first_item  work items (8 columns) before it: per recording 48 + min(4 q, 48) (windows - 1)
 *   [4] q           hop_slots of this recording
 * out[total_slots][64][96], MLA_F32 or MLA_BF16 (one rounding of the f32 value), 16-byte aligned: out[first_slot + r][b][x] =
 * log-mel of band b, column 32 u + x, for the recording's r-th kept slot u; exactly 0.0 for columns >= spec_cols. The layout of
 * mla_logmel_bags' windows: ten consecutive rows from a window's first row ARE its bag, bit for bit. Every element of out is
 * written exactly once; columns in no kept slot (q > 11) get no spectrum; no sample beyond 160 spec_cols + 240 of a row is read.
 * Errors, all before any launch: null pointer, misaligned out, q < 1, (cols, spec_cols) that are no track, first_slot /
 * first_item that are not the sums before them, total_slots that is not the sum -> MLA_E_ARG; a descriptor that reads past
 * n_samples, more than 2^31 - 1 items -> MLA_E_SHAPE; dtype codes -> MLA_E_DTYPE. recordings == 0 returns MLA_OK. */
int mla_logmel_timeline(const void* pcm, int pcm_dtype, int64_t recordings, int64_t n_samples, int64_t row_stride, const int64_t* desc,
                        const int64_t* host_desc, int64_t total_slots, const float* tables, void* out, int out_dtype,
                        mla_stream_t stream);
/* ---- ResNet branch front-end: dataset.create_spec(cnn_type="resnet") + split (dataset.py:309-316, :329-363) ----
 * librosa.feature.melspectrogram(y, sr, n_mels=n_mels, hop_length=hop) with its defaults (n_fft = win_length = 2048,
 * periodic Hann, center=True, pad_mode="reflect", power 2, Slaney mel basis over 0..sr/2, norm="slaney") followed by
 * librosa.power_to_db(S, ref=1.0, amin, top_db), for a batch of clips. n_fft is fixed at 2048 (the reference never
 * passes another); 1 <= n_mels <= 1024; clips of at least 1025 samples (one reflection must cover the 1024-sample
 * padding; shorter clips return MLA_E_SHORT). */

/* Spectrogram columns of a clip: 1 + n_samples / hop (host; -1 for n_samples < 0 or hop < 1). */
int64_t mla_melspec_frames(int64_t n_samples, int64_t hop);
/* Constant tables (periodic Hann, FFT twiddles, the Slaney filterbank in sparse form: per band the first bin, the bin
 * count and the offset of its packed weights), computed in double precision on the host and rounded once.
 * `host_out` receives mla_melspec_table_floats(sr, n_mels) floats (-1 for an invalid configuration); the caller
 * uploads them once per (sr, n_mels) and passes the device copy to mla_melspec_db. */
int64_t mla_melspec_table_floats(double sr, int64_t n_mels);
int     mla_melspec_build_tables(double sr, int64_t n_mels, float* host_out);
/* Bytes of the per-clip partial maxima mla_melspec_db writes and mla_melspec_images reads (-1 for bad arguments). */
int64_t mla_melspec_workspace_bytes(int64_t clips, int64_t n_samples, int64_t hop);
/* pcm[clips][clip_stride] f32 (the first n_samples of each row are used) -> out_db[clips][n_mels][frames],
 * 10 log10(max(amin, S)) WITHOUT the top_db clip, frames = mla_melspec_frames(n_samples, hop), and the workspace of
 * partial maxima. A clip's values depend on its own samples only (fixed summation order, no atomics). */
int mla_melspec_db(const float* pcm, int64_t clips, int64_t n_samples, int64_t clip_stride, int64_t hop, int64_t n_mels,
                   float amin, const float* tables, float* out_db, float* workspace, mla_stream_t stream);
/* power_to_db's clip + split: out[clips][n_images][1][n_mels][image_w] with
 * out[c][t][0][b][x] = max(db[c][b][t * image_stride + x], max(db[c]) - top_db); the maximum is taken over the clip's
 * whole spectrogram (from `workspace`, as mla_melspec_db left it for the same clips, n_samples and hop). Images
 * that leave the spectrogram ((n_images - 1) * image_stride + image_w > frames) are MLA_E_SHAPE.
 * n_images = 1, image_w = frames gives the clipped spectrogram itself. */
int mla_melspec_images(const float* db, const float* workspace, int64_t clips, int64_t n_samples, int64_t hop, int64_t n_mels,
                       float top_db, int64_t n_images, int64_t image_w, int64_t image_stride, float* out, mla_stream_t stream);

/* ---- the gradient of mla_melspec_db + mla_melspec_images with respect to the waveform ----
 * float32, deterministic, no atomics; a clip's gradient depends on that clip alone (not on the batch, the strides or the grid).
 * Errors of the three entries, all before any launch, with the codes and texts of the forward entries: null or misaligned
 * pointer, hop < 1, n_mels outside [1, 1024], a stride < n_samples, amin <= 0, top_db < 0 -> MLA_E_ARG; n_samples < 1025 ->
 * MLA_E_SHORT; images that leave the spectrogram -> MLA_E_SHAPE. clips == 0 returns MLA_OK and touches nothing. */

/* Bytes of the workspace mla_melspec_db_bwd needs: per clip and run of up to 32 frames one span of overlap-added frame gradients
 * (-1 for bad arguments). */
int64_t mla_melspec_bwd_workspace_bytes(int64_t clips, int64_t n_samples, int64_t hop, int64_t n_mels);
/* grad_images[clips][n_images][1][n_mels][image_w] = dL / d out of mla_melspec_images, with the `db` and `workspace` the forward
 * produced for the same clips -> d_db[clips][n_mels][frames] = dL / d db: overlapping images add; a cell below the floor
 * max(db[c]) - top_db passes nothing and a cell above it passes its gradient. With floor_grad != 0 the floor's own gradient, the
 * sum over the clipped cells, is added to the cell that holds the maximum (the first in (band, column) order where several do;
 * torch spreads it evenly); with floor_grad == 0 the floor is a constant. Every element of d_db is stored exactly once. */
int mla_melspec_images_bwd(const float* grad_images, const float* db, const float* workspace, int64_t clips, int64_t n_samples,
                           int64_t hop, int64_t n_mels, float top_db, int64_t n_images, int64_t image_w, int64_t image_stride,
                           int floor_grad, float* d_db, mla_stream_t stream);
/* pcm as mla_melspec_db took it, d_db[clips][n_mels][frames] -> d_pcm[clips][d_stride] = dL / d pcm (the first n_samples of each
 * row are stored, each exactly once: the caller zeroes nothing; nothing at or behind n_samples is touched). The frames' spectra
 * are recomputed from pcm; `tables` are mla_melspec_build_tables' (the transposed mel step needs no table of its own);
 * bwd_workspace holds mla_melspec_bwd_workspace_bytes. A band with S <= amin passes nothing: an all-zero clip gives exact zeros. */
int mla_melspec_db_bwd(const float* pcm, int64_t clips, int64_t n_samples, int64_t clip_stride, int64_t hop, int64_t n_mels,
                       float amin, const float* tables, const float* d_db, float* bwd_workspace, float* d_pcm, int64_t d_stride,
                       mla_stream_t stream);

/* ---- ResNet branch over time: a recording of any length scored in 4 s windows at a hop of hop_images / 3 s ----
 * Extends create_spec(cnn_type="resnet") + split (dataset.py:309-316, :329-363) beyond the reference's loader, which cuts every
 * recording at 4 s (dataset.py:233-237); the configuration is the reference's: 22 050 Hz, 224 bands, hop 98, ten images of 224
 * columns 75 columns apart per 88 200-sample window.
 * Host only, the single source of the arithmetic, exact for any int64 n_samples. An image step is 75 columns = 7 350 samples.
 * With q = hop_images >= 1:
 *   n >= 88 200: windows = 1 + (n - 88 200) / (7 350 q); a trailing stretch that fills no window is dropped;
 *   n <  88 200: one window, the recording zero-filled to 88 200 samples (dataset.py:235-237).
 * The TRACK is the first *samples = 88 200 + 7 350 q (windows - 1) samples, centre-padded by reflection at its own two ends, with
 * *columns = 1 + samples / 98 spectrogram columns; D = power_to_db(melspectrogram(track), top_db=None) and the floor is taken
 * against the TRACK-wide maximum: librosa's spectrogram of the whole track, cut into images. Image u is columns [75 u, 75 u + 224);
 * it is kept iff u mod q < 10 and u <= q (windows - 1) + 9. *images is their number: q (windows - 1) + 10 for q <= 10, where
 * window j is rows q j .. q j + 9 of the recording's kept images, and 10 * windows for q > 10, window j = rows 10 j .. 10 j + 9.
 * Against cropping 4 s pieces on the host (mla_melspec_db + mla_melspec_images per crop), which reflects at each crop's ends and
 * floors against each crop's maximum: columns 0..10 of a window's first image and 890..898 of its last differ, and a window
 * quieter than the track's loudest sits on a higher floor; all else is the same samples through the same arithmetic. One window
 * IS the crop. Any output pointer may be NULL. n_samples < 0, hop_images < 1 or > 2^30 -> MLA_E_ARG. */
int mla_melspec_track_counts(int64_t n_samples, int64_t hop_images, int64_t* windows, int64_t* images, int64_t* samples,
                             int64_t* columns);
/* mla_melspec_db for a RAGGED batch: the unclipped dB spectrogram of every recording's track and its maximum, two launches
 * whatever the batch is. pcm[recordings][row_stride] f32 at 22 050 Hz (the first n_samples of a row are valid input).
 * desc[recordings][6] (DEVICE, int64) and host_desc, the same array on the HOST, read for validation before anything is launched.
 * Per recording:
 *   [0] samples      the track's samples, 88 200 + 7 350 q (windows - 1), at most 2^30
 *   [1] cols         1 + samples / 98
 *   [2] first_run    runs of 16 columns before it: per recording ceil(cols / 16)
 *   [3] db_offset    floats of out_db before it: 224 * the columns before it
 *   [4] first_image  kept images before it (mla_melspec_track_images' rows)
 *   [5] q            hop_images of this recording
 * out_db: total_columns * 224 floats, recording r's block at db_offset, band-major (224, cols). workspace: one float per run
 * (the sum of ceil(cols / 16)), the runs' maxima; maxima[recordings]: max(D_r), NaN if a sample of the track is. `tables`: the
 * device copy of mla_melspec_build_tables(22050, 224). A recording's values depend on its own track only, the same bits alone,
 * in any batch and at any position; columns 11 .. cols - 12 are the bits mla_melspec_db gives any 88 200-sample crop that holds
 * their frames' samples. Nothing at or behind `samples` of a row is read.
 * Errors, all before any launch: null or misaligned pointer, q < 1, (samples, cols) that are no track, prefixes that are not the
 * sums before them, total_columns that is not the sum, amin <= 0 -> MLA_E_ARG; a track longer than n_samples or than 2^30, more
 * than 2^31 - 1 runs -> MLA_E_SHAPE. recordings == 0 returns MLA_OK. */
int mla_melspec_track_db(const float* pcm, int64_t recordings, int64_t n_samples, int64_t row_stride, const int64_t* desc,
                         const int64_t* host_desc, int64_t total_columns, float amin, const float* tables, float* out_db,
                         float* workspace, float* maxima, mla_stream_t stream);
/* mla_melspec_images over the tracks of mla_melspec_track_db (same desc / host_desc / total_columns): the kept images with global
 * row in [first, first + count), so that a caller can make them chunk by chunk,
 *   out[row - first][0][b][x] = max(D_r[b][75 u + x], maxima[r] - top_db)   (max keeps NaN)
 * as float32, out 16-byte aligned. Every element of out is written exactly once.
 * Errors, all before any launch: as mla_melspec_track_db for the descriptors; top_db < 0, first < 0, count < 0 -> MLA_E_ARG; a
 * range that leaves the kept images -> MLA_E_SHAPE. count == 0 returns MLA_OK. */
int mla_melspec_track_images(const float* db, const float* maxima, int64_t recordings, const int64_t* desc, const int64_t* host_desc,
                             int64_t total_columns, float top_db, int64_t first, int64_t count, float* out, mla_stream_t stream);

/* ---- VGGish branch, librosa path: dataset.create_spec(cnn_type="vggish", use_librosa=True) + split (dataset.py:305-307, :316,
 * :329-363): librosa.feature.melspectrogram(y, sr, n_mels=64, hop_length=160, center=False, htk=True, fmin=125, fmax=7500)
 * followed by librosa.power_to_db, for a batch of clips. center=False: no padding, frame f is y[f * hop .. f * hop + 2047],
 * frames = 1 + (n_samples - 2048) / hop; clips shorter than one frame (2048 samples) return MLA_E_SHORT. */

/* The tables of mla_melspec_build_tables for any mel basis librosa.filters.mel(sr, 2048, n_mels, fmin, fmax, htk, norm="slaney")
 * builds: htk != 0 is the HTK scale mel = 2595 log10(1 + hz / 700), htk == 0 the Slaney scale; 0 <= fmin < fmax <= sr / 2.
 * (sr, n_mels, 0, sr / 2, 0) gives mla_melspec_build_tables' tables bit for bit. Same layout, same sparse form (a band without a
 * bin centre inside it has a count of 0); -1 / MLA_E_ARG for an invalid configuration. */
int64_t mla_melspec_band_table_floats(double sr, int64_t n_mels, double fmin, double fmax, int htk);
int     mla_melspec_build_band_tables(double sr, int64_t n_mels, double fmin, double fmax, int htk, float* host_out);
/* Spectrogram columns of a clip without padding: 1 + (n_samples - 2048) / hop (host; -1 for n_samples < 2048 or hop < 1). */
int64_t mla_melspec_nopad_frames(int64_t n_samples, int64_t hop);
/* Bytes of the per-clip partial maxima mla_melspec_nopad_db writes and mla_melspec_nopad_bags reads (-1 for bad arguments). */
int64_t mla_melspec_nopad_workspace_bytes(int64_t clips, int64_t n_samples, int64_t hop);
/* pcm[clips][clip_stride] f32 (the first n_samples of each row are used; nothing else is read) ->
 * out_db[clips][n_mels][frames], 10 log10(max(amin, S)) WITHOUT the top_db clip, frames = mla_melspec_nopad_frames(n_samples, hop),
 * and the workspace of partial maxima. `tables` is the device copy of either builder's tables for n_mels bands and
 * `table_floats` their size (the packed weights are staged in LDS, at most 2050 of them). A clip's values depend on its own
 * samples only: the same bits alone, in any batch and at any position. */
int mla_melspec_nopad_db(const float* pcm, int64_t clips, int64_t n_samples, int64_t clip_stride, int64_t hop, int64_t n_mels,
                         float amin, const float* tables, int64_t table_floats, float* out_db, float* workspace, mla_stream_t stream);
/* mla_melspec_images for the spectrogram and workspace of mla_melspec_nopad_db, written as MLA_F32 or MLA_BF16 (one rounding to
 * nearest even of the float32 value): out[clips][n_images][1][n_mels][image_w],
 * out[c][t][0][b][x] = max(db[c][b][t * image_stride + x], max(db[c]) - top_db). With (10, 96, 32) on 388 columns of 64 bands
 * this is the bag tensor the reference stores (dataset.py:252-255). Errors as mla_melspec_images; another dtype code is MLA_E_DTYPE. */
int mla_melspec_nopad_bags(const float* db, const float* workspace, int64_t clips, int64_t n_samples, int64_t hop, int64_t n_mels,
                           float top_db, int64_t n_images, int64_t image_w, int64_t image_stride, void* out, int out_dtype,
                           mla_stream_t stream);

/* vggish.Postprocessor.postprocess (vggish.py:62-102): PCA, clamp to [-2, 2], 8-bit quantisation
 * (as float). embeddings (rows, 128), pca_eigen_vectors (128, 128), pca_means (128). */
int mla_postprocess(const float* embeddings, const float* pca_eigen_vectors, const float* pca_means, int64_t rows,
                    float* out, mla_stream_t stream);

/* ------------------------------------------------------------------------------------
 * VGGish feature stack: torchvggish/vggish.py:108-118 (make_layers) applied at :22.
 * Activations are NHWC (N, H, W, C) in the compute dtype (MLA_BF16 or MLA_F32); this
 * makes the reference's NCHW->NHWC flatten (vggish.py:26-29, model.py:190-193) a no-op.
 * ---------------------------------------------------------------------------------- */

/* nn.Conv2d weight (Cout, Cin, 3, 3) f32 (state_dict layout) -> (Cout, 9, Cin) in `dtype`,
 * the K-contiguous layout the implicit-GEMM kernels stream. */
int mla_conv_repack_weights(const float* w_oihw, int64_t cout, int64_t cin, void* out, int dtype,
                            mla_stream_t stream);
/* f32 -> bf16 copy (nn.Linear weights for the bf16 GEMMs). */
int mla_convert_f32(const float* in, void* out, int64_t n, int dtype, mla_stream_t stream);
/* bf16 -> f32 copy (bf16 conv bottlenecks feeding the f32 MLA head, model.py:162-167 path). */
int mla_convert_bf16_to_f32(const void* in, float* out, int64_t n, mla_stream_t stream);
/* MLA_BF16X3 operand preparation: float32 (rows, cols) -> bf16 planes per segment of `seg` columns, [hi | lo] (copies = 2:
 * activations) or [hi | lo | hi] (copies = 3: weights; conv weights: rows = Cout*9 of the (Cout, 9, Cin) repack, seg = 64 = one K chunk;
 * Linear weights: seg = the activation's plane length, 512 after the conv stack's NHWC flatten, else in_features). */
int mla_split_bf16x3(const float* in, int64_t rows, int64_t cols, int64_t ld_in, void* out, int64_t ld_out, int64_t seg,
                     int copies, mla_stream_t stream);
/* split (rows, 2 cols) = [hi | lo] per segment -> float32 (rows, cols) = hi + lo (the bottleneck features of
 * just_bottlenecks=True, model.py:162-167, handed to the float32 head). */
int mla_merge_bf16x3(const void* in, int64_t rows, int64_t cols, int64_t ld_in, int64_t seg, float* out, mla_stream_t stream);
/* nn.Linear in the MLA_BF16X3 mode (vggish.py:13-19 at f32-grade accuracy on the bf16 matrix cores): a (M, 2K) split
 * activations, w (N, 3K) from mla_split_bf16x3, K = in_features, seg as above; out_dtype MLA_F32 (M, N) or MLA_BF16X3
 * (M, 2N) = [hi(N) | lo(N)]. */
int mla_linear_bf16x3(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, void* out, int64_t ldo,
                      int64_t M, int64_t N, int64_t K, int64_t seg, int out_dtype, int relu, mla_stream_t stream);

/* features[0..2]: Conv2d(1, 64, 3, pad 1) + ReLU + MaxPool2d(2, 2) fused.
 * x: (n, 96, 64) examples (x_dtype MLA_F32 | MLA_BF16); w: (64, 1, 3, 3) f32; bias (64) f32;
 * out: (n, 48, 32, 64) NHWC in `dtype`. */
int mla_vggish_conv1(const void* x, int x_dtype, int64_t n, const float* w, const float* bias, void* out,
                     int dtype, mla_stream_t stream);

/* mla_logmel_examples (bf16 examples) followed by mla_vggish_conv1 (bf16 in, bf16 out) as ONE kernel: the examples never
 * exist in memory (vggish_input.py:30-82 -> mel_features.py:192-223 -> vggish.py:108-118 features[0..2] applied at :22).
 * pcm / n_wave / n_samples / wave_stride / tables as for mla_logmel_examples, w / bias as for
 * mla_vggish_conv1; out: (n_wave * examples, 48, 32, 64) NHWC bf16, bit-identical to the two calls. */
int mla_logmel_conv1(const void* pcm, int pcm_dtype, int64_t n_wave, int64_t n_samples, int64_t wave_stride,
                     const float* tables, const float* w, const float* bias, void* out, mla_stream_t stream);

/* conv `layer` in 2..6 = features[3], [6], [8], [11], [13], each fused with its ReLU and,
 * for layers 2, 4 and 6, with the MaxPool2d(2, 2) that follows it:
 *   2: (n,48,32, 64) -> (n,24,16,128)     3: (n,24,16,128) -> (n,24,16,256)
 *   4: (n,24,16,256) -> (n,12, 8,256)     5: (n,12, 8,256) -> (n,12, 8,512)
 *   6: (n,12, 8,512) -> (n, 6, 4,512)
 * in / out / w_repacked (from mla_conv_repack_weights) in `dtype`; bias f32. */
int mla_vggish_conv(int layer, const void* in, const void* w_repacked, const float* bias, void* out,
                    int64_t n, int dtype, mla_stream_t stream);

/* torch.nn.Linear (+ optional ReLU): out[M, N] = act(a[M, K] . w[N, K]^T + bias[N]).
 * VGG.embeddings (vggish.py:13-19) and the MLA fc / fcv layers (model.py:207-210, :230).
 * a, w in `dtype` with leading dimensions lda, ldw (elements, 16-byte multiples); out in
 * out_dtype (MLA_F32, or MLA_BF16 when dtype is MLA_BF16); bias f32 or NULL. */
int mla_linear(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, void* out,
               int64_t ldo, int64_t M, int64_t N, int64_t K, int dtype, int out_dtype, int relu,
               mla_stream_t stream);
/* mla_linear for NARROW forward layers with a long reduction (vggish.py:17: Linear(4096, 128)): K is cut into `splits` equal
 * ranges of whole 128-byte stages that run as separate workgroups; the float32 partial sums (workspace: splits * M * N floats)
 * are added in range order, then bias / ReLU. The caller fixes `splits` per LAYER, never per batch: every addition's order
 * depends on (K, splits) only, so a row's result does not depend on the batch it is computed in. f32 or bf16 operands. */
int mla_linear_ksplit(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, void* out, int64_t ldo,
                      int64_t M, int64_t N, int64_t K, int dtype, int out_dtype, int relu, int splits, float* workspace,
                      int64_t workspace_floats, mla_stream_t stream);
/* mla_linear in f32 with the reduction dimension split over `splits` workgroup ranges (weight
 * gradients: few output tiles, K = batch rows); partial sums go through workspace
 * (splits * M * N floats) and are combined in fixed order. */
int mla_linear_splitk(const float* a, int64_t lda, const float* w, int64_t ldw, const float* bias, float* out,
                      int64_t ldo, int64_t M, int64_t N, int64_t K, int relu, int splits, float* workspace,
                      int64_t workspace_floats, mla_stream_t stream);
/* nn.Linear with a NARROW output (N <= 16; model.py:230 fcv: 600 -> 10): one pass over `a`, 16 lanes per row, weights in LDS.
 * f32; K % 4 == 0, rows 16-byte aligned, K * N * 4 <= 64 KiB. Every row is computed the same way whatever M. */
int mla_linear_narrow(const float* a, int64_t lda, const float* w, int64_t ldw, const float* bias, float* out,
                      int64_t ldo, int64_t M, int64_t N, int64_t K, mla_stream_t stream);
/* Same contract in f32 without alignment requirements, for tiny layers (model.py:255 fc). */
int mla_linear_small(const float* a, int64_t lda, const float* w, int64_t ldw, const float* bias,
                     float* out, int64_t ldo, int64_t M, int64_t N, int64_t K, mla_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Multi-level attention head: model.py:200-269 (f32 throughout)
 * ---------------------------------------------------------------------------------- */

/* torch.nn.BatchNorm1d batch statistics (train mode). x: (rows, cols) f32, leading dim ldx.
 *   mode 0: channel = row % period  -- BatchNorm1d(T) on a (B, T, F) tensor flattened to
 *           (B*T, F) (model.py:205, :213, :232-233): statistics over (batch, feature) per slot;
 *   mode 1: channel = column        -- BatchNorm1d(K) on (B, K) (model.py:256).
 * Writes mean and BIASED variance (what normalisation uses); if running_mean/var are non-NULL
 * and momentum >= 0 they are updated in place with the UNBIASED variance, as torch does.
 * Limits: mode 0 period 1..64 (rows a multiple of it); mode 1 cols 1..1024 (above 64 columns a kernel of its own; up to 64
 * the launches and bits are what they were). Anything else: MLA_E_SHAPE. The same limits hold for the two-stage and fused
 * forms below. The backward pair mla_bn_bwd_sums / mla_bn_bwd_apply keeps 64 columns as its mode-1 limit; wider layers go
 * through mla_bn_bwd_sums_wide / mla_bn_bwd_apply_wide.
 * workspace: mla_bn_stats_workspace_bytes() bytes of device memory. Deterministic. */
int64_t mla_bn_stats_workspace_bytes(void);
int mla_bn_stats(const float* x, int64_t rows, int64_t cols, int64_t ldx, int mode, int period,
                 void* workspace, float* mean, float* var_biased, float* running_mean,
                 float* running_var, float momentum, mla_stream_t stream);

/* y = act((x - mean[c]) / sqrt(var[c] + eps) * gamma[c] + beta[c]), then optional dropout:
 * y = keep_mask ? y * drop_scale : 0 (keep_mask: rows*cols bytes or NULL). act: 0 none, 1 ReLU
 * (model.py:219), 2 sigmoid (model.py:268). Channel modes as mla_bn_stats. In eval mode the
 * caller passes the running statistics, in train mode the batch statistics. */
int mla_bn_apply(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int64_t cols, int mode,
                 int period, const float* mean, const float* var, const float* gamma, const float* beta,
                 float eps, int act, const uint8_t* keep_mask, float drop_scale, mla_stream_t stream);

/* model.AttentionModule.forward (model.py:236-242) after the fcv Linear: z (bags*T, K) ->
 * y (bags, K) written with leading dimension ldy (so levels concatenate in place,
 * model.py:267). BatchNorm parameters of normv (v_*) and normf (f_*) per time slot (T values).
 * att_out / cla_out (bags*T*K each) receive softmax / sigmoid for the backward pass, or NULL.
 * Limits: 1 <= T <= 64, 1 <= K <= 1024, else MLA_E_SHAPE. T, K <= 16: 16 lanes per bag, the classes in registers; wider bags
 * take one workgroup each. Either way a bag's result does not depend on the batch it sits in or on att_out / cla_out, and
 * mla_attention_pool_bwd has the same limits and dispatch. */
int mla_attention_pool(const float* z, int64_t bags, int T, int K, const float* v_mean, const float* v_var,
                       const float* v_gamma, const float* v_beta, const float* f_mean, const float* f_var,
                       const float* f_gamma, const float* f_beta, float eps, float* y, int64_t ldy,
                       float* att_out, float* cla_out, mla_stream_t stream);

/* Bags of T consecutive rows out of shared embeddings: out[(w T + t)][m] = emb[first_row[w] + t][m], m < M. emb (rows, M; leading
 * dimension ld), out (windows * T, M) contiguous, both f32; first_row[windows] (DEVICE, int64) and host_first_row, the same on the
 * HOST for validation. Windows may overlap (a timeline's do). BatchNorm1d(T) of the head is per slot position, so only the CNN is
 * shared between windows, not the head. 16-byte accesses where M, ld and both pointers allow, scalar ones otherwise.
 * Errors: negative sizes, T < 1, M < 1, ld < M, null pointers, a window that leaves emb -> MLA_E_ARG. windows == 0 returns MLA_OK. */
int mla_gather_bags(const float* emb, int64_t rows, int64_t ld, const int64_t* first_row, const int64_t* host_first_row,
                    int64_t windows, int T, int64_t M, float* out, mla_stream_t stream);

/* Two-stage form of mla_bn_stats for data-parallel training: stage 1 writes the LOCAL
 * per-channel (sum x, sum x^2) as 2*channels doubles; the host side may all-reduce them over
 * ranks (SyncBN: the reference's single process sees the global batch); stage 2 turns sums +
 * per-channel element count into mean / biased variance (+ running update). */
int mla_bn_stats_sums(const float* x, int64_t rows, int64_t cols, int64_t ldx, int mode, int period,
                      void* workspace, double* sums, mla_stream_t stream);
int mla_bn_stats_finish(const double* sums, int channels, double count, float* mean, float* var_biased,
                        float* running_mean, float* running_var, float momentum, int64_t* num_batches_tracked /* += 1, or NULL */,
                        mla_stream_t stream);
/* Both stages for a single process (no all-reduce in between) in two launches instead of three; same results bit for bit.
 * sums_out: the 2*channels doubles of stage 1 (for a second BatchNorm fed by the same tensor, model.py:237-238). */
int mla_bn_stats_fused(const float* x, int64_t rows, int64_t cols, int64_t ldx, int mode, int period, void* workspace,
                       double* sums_out, float* mean, float* var_biased, float* running_mean, float* running_var,
                       float momentum, int64_t* num_batches_tracked, mla_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Training step: train.py:124-138 (zero_grad, forward, CrossEntropyLoss, backward, Adam)
 * ---------------------------------------------------------------------------------- */

/* BatchNorm1d backward (train mode), through the activation/dropout fused in mla_bn_apply:
 * g = dy taken through act (1: ReLU[+dropout] using the forward output yout, 2: sigmoid, 0: none).
 * Stage 1: LOCAL per-channel (sum g, sum g*xhat) as 2*channels doubles (all-reducible).
 * Stage 2: dx = gamma*inv*(g - sum g/N - xhat*sum(g xhat)/N) from the GLOBAL sums and count N
 * (written, or added when accumulate != 0; NULL to skip) and dgamma/dbeta from the LOCAL sums
 * (the gradient all-reduce adds the ranks' parts; NULL to skip). */
int mla_bn_bwd_sums(const float* x, int64_t ldx, const float* dy, int64_t ld_dy, const float* yout, int64_t ld_y,
                    int act, float drop_scale, int64_t rows, int64_t cols, int mode, int period, const float* mean,
                    const float* var, float eps, void* workspace, double* sums, mla_stream_t stream);
int mla_bn_bwd_apply(const float* x, int64_t ldx, const float* dy, int64_t ld_dy, const float* yout, int64_t ld_y,
                     int act, float drop_scale, int64_t rows, int64_t cols, int mode, int period, const float* mean,
                     const float* var, const float* gamma, float eps, const double* sums_global,
                     const double* sums_local, double count, float* dx, int64_t ld_dx, int accumulate,
                     float* dgamma, float* dbeta, mla_stream_t stream);
/* The same two stages in column mode (channel = column; BatchNorm1d(K), model.py:256) for 1 <= cols <= 1024, without the
 * mode / period arguments. Up to 64 columns: the launches and bits of the pair above. workspace as mla_bn_stats. */
int mla_bn_bwd_sums_wide(const float* x, int64_t ldx, const float* dy, int64_t ld_dy, const float* yout, int64_t ld_y,
                         int act, float drop_scale, int64_t rows, int64_t cols, const float* mean, const float* var,
                         float eps, void* workspace, double* sums, mla_stream_t stream);
int mla_bn_bwd_apply_wide(const float* x, int64_t ldx, const float* dy, int64_t ld_dy, const float* yout, int64_t ld_y,
                          int act, float drop_scale, int64_t rows, int64_t cols, const float* mean, const float* var,
                          const float* gamma, float eps, const double* sums_global, const double* sums_local, double count,
                          float* dx, int64_t ld_dx, int accumulate, float* dgamma, float* dbeta, mla_stream_t stream);

/* Backward of mla_attention_pool: dy (bags, K; leading dim ld_dy) and the saved att / cla ->
 * gradients w.r.t. the normv output (du_v) and the normf output (du_f), (bags*T, K) each. */
int mla_attention_pool_bwd(const float* dy, int64_t ld_dy, const float* att, const float* cla, int64_t bags, int T,
                           int K, float* du_v, float* du_f, mla_stream_t stream);

/* Backward of mla_linear_small: da (M, K) = dz . w, dw (N, K) = dz^T . a, db (N) = column sums. */
int mla_linear_small_bwd(const float* a, int64_t lda, const float* w, int64_t ldw, const float* dz, int64_t ldz,
                         int64_t M, int64_t N, int64_t K, float* da, int64_t ldda, float* dw, float* db,
                         mla_stream_t stream);

/* out[c][r] = in[r][c] (f32). The Linear backward feeds the K-contiguous MFMA GEMM with
 * transposed copies: dX = mla_linear(dZ, W^T), dW = mla_linear(dZ^T, X^T). */
int mla_transpose_f32(const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t rows, int64_t cols,
                      mla_stream_t stream);
/* out[c] = sum_r x[r][c] (bias gradients). workspace: 64 * cols doubles. Deterministic. */
int mla_col_sum(const float* x, int64_t ldx, int64_t rows, int64_t cols, void* workspace, float* out,
                mla_stream_t stream);
/* y += a * x */
int mla_axpy(float a, const float* x, float* y, int64_t n, mla_stream_t stream);

/* nn.CrossEntropyLoss (train.py:372) on scores x (rows, K) with int64 labels: writes
 * loss = inv_total * sum_b (logsumexp(x_b) - x_b[y_b]) and, if dx != NULL,
 * dx = inv_total * (softmax(x_b) - onehot(y_b)); n_correct (optional, TWO ints): [0] = #argmax hits
 * (train.py:133), [1] = #labels outside [0, K) -- those rows contribute neither loss nor gradient, and the loss is NaN
 * when there is one (nn.CrossEntropyLoss raises; the caller does, on reading [1]). Two separate counters so that a sum
 * over data-parallel ranks cannot cancel one against the other. inv_total = 1 / global batch (mean over all ranks). */
int mla_cross_entropy(const float* x, int64_t ldx, const int64_t* labels, int64_t rows, int K, float inv_total,
                      float* loss, float* dx, int64_t ld_dx, int* n_correct, mla_stream_t stream);

/* nn.CrossEntropyLoss with its options, beside mla_cross_entropy (which stays the plain criterion's kernel): class weights
 * (weight: K floats on the device, NULL = all ones), label_smoothing in [0, 1], ignore_index, reduction 0 = mean | 1 = sum.
 * A row whose label equals ignore_index adds nothing: no loss, exact zeros in dx, neither a hit nor a bad label. K <= 1024.
 *   mla_cross_entropy_den : den[0] = sum of weight[y_b] over the rows with an in-range label other than ignore_index (one
 *     workgroup, double precision, fixed order). Labels and weights only: a data-parallel step sums den over its ranks before
 *     the main call, so that the mean is the global batch's.
 *   mla_cross_entropy_opts: one wavefront per row; the row terms go to `workspace` (mla_cross_entropy_opts_workspace_bytes(rows)
 *     bytes, 8-byte aligned) and one workgroup adds them in double in a fixed order: no atomics, bit-reproducible. The mean's
 *     scale 1 / den[0] is read from DEVICE memory (den: NULL for the sum), so the sequence replays in a HIP graph. dx may be
 *     NULL. counts = THREE ints [#argmax hits, #labels outside [0, K) other than ignore_index, #labels other than
 *     ignore_index]; a label outside [0, K) is never used as an index, its dx row is zero and the loss is NaN. With no
 *     counted row the mean is NaN (0 / 0, as torch) and the sum 0. */
int mla_cross_entropy_den(const int64_t* labels, int64_t rows, int K, const float* weight, int64_t ignore_index, float* den,
                          mla_stream_t stream);
int64_t mla_cross_entropy_opts_workspace_bytes(int64_t rows);
int mla_cross_entropy_opts(const float* x, int64_t ldx, const int64_t* labels, int64_t rows, int K, const float* weight,
                           int64_t ignore_index, float label_smoothing, int reduction, const float* den, float* loss, float* dx,
                           int64_t ld_dx, int* counts, void* workspace, mla_stream_t stream);

/* nn.BCELoss(weight, reduction) on probabilities p (rows, K <= 1024; the head's sigmoid outputs) with float32 targets (rows, K) in
 * [0, 1], soft targets included: the criterion of a multi-label step.
 *   term = w_k ((y - 1) max(log(1 - p), -100) - y max(log p, -100)),  loss = s * sum term,
 *   dp = s w_k (p - y) / max((1 - p) p, 1e-12),  s = scale under reduction 0 (mean; pass 1 / (GLOBAL rows * K)), 1 under 1 (sum).
 * weight: K floats on the device, NULL = all ones. dp may be NULL (loss and counters only, the same loss bits). One wavefront
 * per row, the row terms go to `workspace` (mla_bce_workspace_bytes(rows) bytes, 8-byte aligned) and one workgroup adds them in
 * double in a fixed order: no atomics, bit-reproducible; every scalar is a launch argument, so the pair replays in a HIP graph.
 * A cell whose target is NaN or outside [0, 1], or whose p lies outside [0, 1], is BAD (torch raises): no logarithm is taken,
 * its dp is an exact zero and the loss is NaN. A NaN in p travels into the loss and into its own cell of dp.
 * counts = THREE ints, both sides thresholded at 0.5: [rows with every class on the right side (subset accuracy), bad cells,
 * cells on the right side]; a bad cell is never right. */
int64_t mla_bce_workspace_bytes(int64_t rows);
int mla_bce(const float* p, int64_t ldp, const float* target, int64_t ldt, int64_t rows, int K, const float* weight, int reduction,
            float scale, float* loss, float* dp, int64_t ld_dp, int* counts, void* workspace, mla_stream_t stream);

/* --- finetune: gradients of the VGGish feature stack (train.py:96-97, :137), f32, NHWC ------ */

/* Generic 3x3/pad-1 convolution entry over the compiled shape set (VGGish forward with or
 * without the fused 2x2 pool, and the five dgrad shapes): act != 0 -> bias + ReLU epilogue,
 * act == 0 -> plain store (transposed convolution; bias may be NULL). dtype MLA_F32 or MLA_BF16
 * (activations and repacked weights in that type, f32 accumulation). */
int mla_conv3x3(const void* in, const void* w_packed, const float* bias, void* out, int64_t n, int H, int W,
                int cin, int cout, int pool, int act, int dtype, mla_stream_t stream);
/* Training forward of a POOLED layer (conv2 / conv4 / conv6 shapes): bias + ReLU, writes BOTH the pre-pool activation
 * (n, H, W, cout) -- kept for the pool / ReLU backward -- and its 2x2 max-pool (n, H/2, W/2, cout) from one pass (the separate
 * mla_maxpool2x2 over the tensor just written is not needed). dtype MLA_F32 or MLA_BF16. */
int mla_conv3x3_train(const void* in, const void* w_packed, const float* bias, void* out_prepool, void* out_pooled, int64_t n,
                      int H, int W, int cin, int cout, int dtype, mla_stream_t stream);
/* (Cout, Cin, 3, 3) -> (Cin, 9, Cout), taps flipped: weights of the dgrad convolution. */
int mla_conv_repack_dgrad(const float* w_oihw, int64_t cout, int64_t cin, float* out, mla_stream_t stream);
/* nn.MaxPool2d(2, 2) on a kept NHWC activation (n, H, W, C) -> (n, H/2, W/2, C). */
int mla_maxpool2x2(const float* a, float* out, int64_t n, int H, int W, int C, mla_stream_t stream);
/* dZ (n, H, W, C) from the gradient of the layer output: pool != 0: d_out is (n, H/2, W/2, C),
 * routed to the first maximum of each window of `a` (kept pre-pool, post-ReLU activation) and
 * masked by ReLU; pool == 0: dZ = d_out * (a > 0). */
int mla_relu_pool_bwd(const float* a, const float* d_out, float* dz, int64_t n, int H, int W, int C, int pool,
                      mla_stream_t stream);
/* the same plus the layer's bias gradient db[C] = column sums of dZ (nn.Conv2d bias, loss.backward() train.py:137), summed
 * on the way in double precision; workspace: mla_relu_pool_bwd_bias_workspace_bytes() bytes */
int64_t mla_relu_pool_bwd_bias_workspace_bytes(void);
int mla_relu_pool_bwd_bias(const float* a, const float* d_out, float* dz, int64_t n, int H, int W, int C, int pool,
                           void* workspace, float* db, mla_stream_t stream);
/* dW (Cout, Cin, 3, 3) = sum over pixels of dZ (n,H,W,Cout) x shifted a_in (n,H,W,Cin); f32 MFMA,
 * deterministic split reduction. workspace: mla_conv_wgrad_workspace_floats() floats. */
int64_t mla_conv_wgrad_workspace_floats(void);
int mla_conv_wgrad(const float* dz, const float* a_in, int64_t n, int H, int W, int cin, int cout, float* workspace,
                   int64_t workspace_floats, float* dw_oihw, mla_stream_t stream);
/* Backward of features[0..2] (Conv2d(1,64)+ReLU+MaxPool): x (n,96,64), d_pooled (n,48,32,64) ->
 * dw (64,1,3,3), db (64). workspace: 1024*8*80 floats. */
int mla_conv1_bwd(const float* x, const float* w, const float* bias, const float* d_pooled, int64_t n, float* workspace,
                  float* dw, float* db, mla_stream_t stream);

/* --- the same backward in bf16 (activations and gradients bf16, f32 accumulation, f32 weight / bias gradients):
 *     what the finetune step runs in at speed; weights stay f32 masters, bf16 copies are re-derived after each Adam step --- */
int mla_conv_repack_dgrad_bf16(const float* w_oihw, int64_t cout, int64_t cin, void* out_bf16, mla_stream_t stream);
int mla_maxpool2x2_bf16(const void* a, void* out, int64_t n, int H, int W, int C, mla_stream_t stream);
/* dZ (bf16) as mla_relu_pool_bwd; a / d_out both bf16 or both f32 (the last Linear's f32 output). db != NULL: also the bias
 * gradient (column sums of dZ, double-precision partials in `workspace` of mla_relu_pool_bwd_bf16_workspace_bytes()). */
int64_t mla_relu_pool_bwd_bf16_workspace_bytes(void);
int mla_relu_pool_bwd_bf16(const void* a, int a_dtype, const void* d_out, int d_dtype, void* dz, int64_t n, int H, int W,
                           int C, int pool, void* workspace, float* db, mla_stream_t stream);
/* dW f32 (Cout, Cin, 3, 3) from bf16 dZ and bf16 a_in on v_mfma_f32_16x16x32_bf16 (operands through the transposing LDS
 * read ds_read_b64_tr_b16); workspace as mla_conv_wgrad. */
int mla_conv_wgrad_bf16(const void* dz, const void* a_in, int64_t n, int H, int W, int cin, int cout, float* workspace,
                        int64_t workspace_floats, float* dw_oihw, mla_stream_t stream);
/* conv1 backward with the incoming gradient in bf16: recompute and weight-gradient products on the matrix cores (patch GEMM, see
 * cnn_train_bf16.hip). workspace: mla_conv1_bwd_workspace_floats() floats (also enough for mla_conv1_bwd). */
/* Training forward of a pooled layer, compact form: instead of the pre-pool activation of mla_conv3x3_train, one BYTE per pooled element
 * (N, H/2, W/2, Cout) -- the window position 0..3 of the first maximum in nn.MaxPool2d's order, or 4 where the ReLU is off -- which is all
 * autograd's backward of `MaxPool2d(ReLU(conv))` (vggish.py:108-118 under train.py:137) needs from that tensor; and the backward that
 * consumes it: dZ (N, H, W, C) bf16 from the codes and the pooled gradient, db on the way (workspace as mla_relu_pool_bwd_bf16). */
int mla_conv3x3_train_codes(const void* in, const void* w_packed, const float* bias, void* out_codes_u8, void* out_pooled, int64_t n,
                            int H, int W, int cin, int cout, int dtype, mla_stream_t stream);
int mla_pool_bwd_codes_bf16(const void* codes_u8, const void* d_pooled_bf16, void* dz_bf16, int64_t n, int H, int W, int C, void* workspace,
                            float* db, mla_stream_t stream);
int mla_conv1_bwd_bf16(const float* x, const float* w, const float* bias, const void* d_pooled_bf16, int64_t n, float* workspace,
                       float* dw, float* db, mla_stream_t stream);
int64_t mla_conv1_bwd_workspace_floats(void);
/* Gradient of features[0..2] (Conv2d(1,64)+ReLU+MaxPool) with respect to its INPUT: x (n,96,64) f32, w (64,1,3,3), bias (64),
 * d_pooled (n,48,32,64) in d_dtype MLA_F32 or MLA_BF16 (16-byte aligned) -> dx (n,96,64) f32, every element written once (dx need
 * not be zeroed). The layer is recomputed under mla_conv1_bwd's rules: bias after the pool, the first maximum in scan order takes
 * the gradient, nothing flows where the pooled output is <= 0; with MLA_BF16, x and w are rounded to bf16 for the recompute as the
 * bf16 forward rounds them. Deterministic (no atomics, the bits do not depend on n), no workspace. n == 0 is a no-op. */
int mla_conv1_dgrad(const float* x, const float* w, const float* bias, const void* d_pooled, int d_dtype, int64_t n, float* dx,
                    mla_stream_t stream);
/* (rows, cols) bf16 -> (cols, ld_out >= rows) bf16, the padding columns zeroed: K-contiguous operands of the Linear backward */
int mla_transpose_bf16(const void* in, int64_t ld_in, void* out, int64_t ld_out, int64_t rows, int64_t cols, mla_stream_t stream);
/* column sums of a bf16 (rows, cols) matrix -> f32 (bias gradient of a Linear); workspace: 64 * cols doubles */
int mla_col_sum_bf16(const void* x, int64_t ldx, int64_t rows, int64_t cols, void* workspace, float* out, mla_stream_t stream);

/* torch.optim.Adam step t (train.py:369; no weight decay, no amsgrad) over one flat buffer. */
int mla_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                  float eps, int64_t step, mla_stream_t stream);
/* The same step with its two step-dependent scalars read from device memory (scal2_dev[0] = lr / (1 - beta1^t), [1] = 1 / sqrt(1 -
 * beta2^t)), so that a HIP graph holding the launch replays train.py:138 with the step count of the moment (the host form bakes
 * them into the launch). mla_adam_prepare writes them for step t, computed on the host exactly as mla_adam_step does: enqueue it
 * in front of every replay. */
int mla_adam_prepare(float* scal2_dev, float lr, float beta1, float beta2, int64_t step, mla_stream_t stream);
int mla_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float beta1, float beta2, float eps,
                      const float* scal2_dev, mla_stream_t stream);

/* torch.optim.Adam / AdamW WITH parameter groups over the same flat buffers (the reference builds `optimizer` at 1e-3 and
 * `optimizer_ft` at 1e-4, train.py:369-371, and stops there; the finetuning recipe needs a learning rate per group, weight decay
 * on weights only, amsgrad, gradient clipping). One launch for all groups.
 *
 * The flat buffers hold the tensors in named_parameters() order, each padded to a multiple of 4 floats. mla_adam_groups_table
 * (host only, no device) turns the tensors' sizes and group indices into the int64 table the kernel reads: maximal runs of
 * adjacent tensors of one group, the run each chunk of the buffer starts in, and the padding quads. Call it with table = NULL
 * for the sizes: counts5 = [padded total, runs, padding entries, chunks, table words]; then with room for the words, and copy
 * them to the device once. More than 64 groups (or none): MLA_E_SHAPE. */
typedef struct {
    float lr, beta1, beta2, eps, weight_decay;
    int decoupled;                      /* AdamW: p <- p (1 - lr wd) before the update; 0: L2, g <- g + wd p */
    int amsgrad;                        /* denominator from the running maximum of v (needs the vmax buffer)  */
} mla_adam_group_t;
int mla_adam_groups_table(const int64_t* numel, const int32_t* group, int64_t n_tensors, int n_groups, int64_t* table,
                          int64_t capacity, int64_t* counts5);
/* Writes the n_groups x 8 float rows the grouped step reads (lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), beta1, beta2, eps, the
 * decay coefficient, flags) for step t. `groups` is HOST memory, read during the call; the values are computed on the host in
 * double, exactly as mla_adam_prepare computes its pair, and travel as a kernel argument: an ordinary launch, no copy, no
 * synchronisation -- enqueue it in front of every step or graph replay, so a changed lr takes effect without a re-capture.
 * groups_dev: 16-byte aligned. More than 64 groups: MLA_E_SHAPE. */
int mla_adam_groups_prepare(float* groups_dev, const mla_adam_group_t* groups, int n_groups, int64_t step, mla_stream_t stream);
/* The step (train.py:138 with torch's options). n = padded total, a multiple of 4; all buffers 16-byte aligned. vmax: the amsgrad
 * maximum, touched by amsgrad groups only (NULL when no group asks for it). coef_dev: NULL, or mla_grad_norm's coefficient: the
 * update then uses coef * g; g itself is only read. Padding elements are never written. With one group, no decay, no amsgrad and
 * coef_dev = NULL the result equals mla_adam_step bit for bit. Graph-capturable: everything step-dependent is device memory. */
int mla_adam_grouped_step(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, const int64_t* table_dev,
                          int64_t table_words, int64_t n_runs, int64_t n_pads, const float* groups_dev, int n_groups,
                          const float* coef_dev, mla_stream_t stream);
/* torch.nn.utils.clip_grad_norm_'s two numbers for the flat gradient: norm_coef_dev[0] = ||g||_2, [1] = min(1, max_norm /
 * (norm + 1e-6)) (NaN for a NaN norm, as torch.clamp gives). Deterministic: sums of squares in double, per block and then over
 * the blocks, in an order that depends on n only; no float atomics. g: 16-byte aligned, read once. workspace:
 * mla_grad_norm_workspace_bytes() bytes. Graph-capturable. */
int64_t mla_grad_norm_workspace_bytes(void);
int mla_grad_norm(const float* g, int64_t n, float max_norm, void* workspace, float* norm_coef_dev, mla_stream_t stream);
/* *counter_dev += delta: the call counter mla_dropout_mask_dev reads, advanced once per step from inside the graph */
int mla_counter_add(int64_t* counter_dev, int64_t delta, mla_stream_t stream);

/* vggish_input.py:52-53 `resampy.resample(data, sample_rate, 16000)`: band-limited sinc interpolation (resampy/interpn.py)
 * of a mono float32 waveform. win / delta: DEVICE tables of the interpolation filter in double precision (right half of the
 * windowed sinc, `num_table` entries per zero crossing, already scaled by the ratio when it is < 1; delta[i] = win[i+1] - win[i],
 * 0 for the last) -- host-side setup like the mel matrix (the package builds resampy's published 'kaiser_best' design).
 * n_out must equal mla_resample_length() = int(n_in * sr_out / sr_in); MLA_E_SHORT if that is 0 (resampy raises ValueError).
 * Parity with resampy itself is UNPINNED (the dependency is absent here): DESIGN.md section 5. */
int64_t mla_resample_length(int64_t n_in, double sr_in, double sr_out);
int mla_resample(const float* x, int64_t n_in, double sr_in, double sr_out, const double* win, const double* delta, int nwin,
                 int num_table, float* y, int64_t n_out, mla_stream_t stream);

/* ---- recordings -> the ResNet branch's clips (dataset.py:232-237: librosa.load(path, sr=22050), cut at 4 s, zero fill) ----
 * ONE launch turns a batch of ragged recordings of any rate and channel count into out[clips][samples_num] float32 at sr_out.
 * packed: DEVICE buffer of packed_elems int16 or float32 elements (pcm_dtype MLA_I16: scaled by 1/32768; MLA_F32), the
 * recordings' interleaved frames back to back (gaps are allowed and never read). Per-clip descriptors, DEVICE arrays of
 * `clips` entries: offsets (element index of the clip's first sample), frames, channels (>= 1), rates (Hz), table_index.
 * The host_* arrays are HOST copies of the same values: every error is decided from them before any launch, and the
 * dynamic LDS is sized from their largest rate.
 *   mono[j] = float(mean over channels in double * scale)                       (mla_mono_mix's arithmetic)
 *   rate == sr_out: out[c][t] = mono[t], t < min(frames, samples_num)           (a copy: the filter is no identity)
 *   otherwise: ratio = sr_out / rate, out[c][t] = resample(mono)[t], t < min(int(frames * ratio), samples_num), bit for bit
 *   what mla_resample computes for the WHOLE recording (the cut comes after the filter); every other element is 0.0f.
 * Every element of out is written. tables: DEVICE, n_tables filter tables back to back, each nwin (win, delta) PAIRS of
 * doubles (win already scaled by the ratio where it is < 1, as for mla_resample); table_index selects a clip's table and is
 * ignored for clips at sr_out. MLA_E_ARG: null pointer with clips > 0, negative size, channels < 1, rate <= 0, unknown
 * pcm_dtype, a clip that leaves the packed buffer, a table index outside [0, n_tables). MLA_E_SHAPE: a rate above
 * 16 * sr_out (a workgroup stages its input span in LDS), a ratio below the table's resolution (int(ratio * num_table) < 1).
 * MLA_E_SHORT: int(frames * ratio) < 1 (resampy raises ValueError). clips == 0 returns MLA_OK and touches nothing.
 * mla_clips_lds_bytes: the dynamic LDS the launch takes for these rates (host; a negative MLA_E_* code for the rate errors
 * above). */
int64_t mla_clips_lds_bytes(const double* host_rates, int64_t clips, double sr_out, int nwin, int num_table);
int mla_clips_prepare(const void* packed, int pcm_dtype, int64_t packed_elems, int64_t clips, const int64_t* offsets,
                      const int64_t* frames, const int32_t* channels, const double* rates, const int32_t* table_index,
                      const int64_t* host_offsets, const int64_t* host_frames, const int32_t* host_channels,
                      const double* host_rates, const int32_t* host_table_index, double sr_out, int64_t samples_num,
                      const double* tables, int64_t n_tables, int nwin, int num_table, float* out, mla_stream_t stream);
/* mla_clips_prepare for recordings that still are the BYTES of their files' data chunks (little endian, interleaved), so that
 * a batch of 8/16/24/32-bit PCM, float32 and float64 files is uploaded as it sits on disk and decoded in the same ONE launch.
 * packed: DEVICE buffer of packed_bytes bytes, aligned to 8. offsets are BYTE offsets; formats (DEVICE) / host_formats hold a
 * sample format code per clip; everything else is mla_clips_prepare's, argument for argument.
 *   code      file encoding                  value summed over the channels            scale after the mean
 *   MLA_U8    unsigned 8-bit                 x - 128                                   1 / 128
 *   MLA_I16   signed 16-bit                  x                                         1 / 32768
 *   MLA_I24   signed 24-bit, 3 packed bytes  x, sign-extended                          1 / 8388608
 *   MLA_I32   signed 32-bit                  x                                         1 / 2147483648
 *   MLA_F32   IEEE float32                   x                                         1
 *   MLA_F64   IEEE float64                   double(float(x)): rounded per sample      1
 *   mono[j] = float(sum in double / channels * scale): mla_clips_prepare's mix. MLA_I16 and MLA_F32 clips give its rows bit for
 *   bit, and every format gives its rows on the samples decoded to float32 first wherever those are exact (all but
 *   multi-channel MLA_I32, whose integers are summed exactly and rounded once).
 * No byte outside [offset, offset + frames * channels * bytes_per_sample) of a clip is read: 24-bit samples are assembled from
 * their bytes, the 2/4/8-byte formats use naturally aligned loads. MLA_E_ARG in addition to mla_clips_prepare's: an unknown
 * format code, an offset that is no multiple of the clip's sample size, a packed pointer that is not aligned to 8 bytes. */
int mla_clips_prepare_raw(const void* packed, int64_t packed_bytes, int64_t clips, const int64_t* offsets, const int64_t* frames,
                          const int32_t* channels, const double* rates, const int32_t* table_index, const int32_t* formats,
                          const int64_t* host_offsets, const int64_t* host_frames, const int32_t* host_channels,
                          const double* host_rates, const int32_t* host_table_index, const int32_t* host_formats, double sr_out,
                          int64_t samples_num, const double* tables, int64_t n_tables, int nwin, int num_table, float* out,
                          mla_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Data-parallel exchange (the reference is single-process, train.py:119-142: these entry
 * points are what makes its step run sharded over the GPUs of a node) and the dropout masks of the step.
 * ---------------------------------------------------------------------------------- */

/* RCCL communicator of this process' rank. The library binds the RCCL ALREADY LOADED in the process (dlopen NOLOAD: the one
 * PyTorch ships, or the host's own; ROCm's librccl.so.1 only if none is loaded) -- it never links a second one.
 * mla_comm_unique_id: rank 0 fills a 128-byte HOST buffer (ncclGetUniqueId) and distributes it by the host's own means;
 * mla_comm_init_rank: every rank, with its HIP device current (ncclCommInitRank; blocks until all ranks have called);
 * an ncclComm_t the host created itself may be passed as `comm` to mla_allreduce_flat unchanged. */
int         mla_comm_unique_id(void* id_host_128);
int         mla_comm_init_rank(void** comm_out, int nranks, const void* id_host_128, int rank);
int         mla_comm_destroy(void* comm);
int         mla_comm_count(void* comm, int* count);   /* ncclCommCount: the number of ranks the communicator spans */
const char* mla_comm_library_origin(void);   /* "already loaded by the host" | "loaded by libmla_hip" | "none" */

/* In-place sum over the ranks of `comm` of a flat device buffer (ncclAllReduce, ncclSum), enqueued on `stream`:
 * the gradient buffer (or one bucket of it) of loss.backward() (train.py:137) before optimizer.step() (train.py:138),
 * the SyncBN (sum, sum of squares) doubles of mla_bn_stats_sums / mla_bn_bwd_sums, the loss and n_correct.
 * dtype: MLA_F32, MLA_F64 or MLA_I32. */
int mla_allreduce_flat(void* buf, int64_t count, int dtype, void* comm, mla_stream_t stream);

/* nn.Dropout(p) keep-mask (model.py:213, 1 = keep), counter-based so that it is reproducible and shardable: element i
 * of the GLOBAL tensor gets 1 iff hash24(seed, stream_id, offset + i) >= round(p_drop * 2^24), hash24 = top 24 bits of
 * the splitmix64 finaliser over (seed, stream_id, index) (bit-exact numpy restatement: <pkg>/weights.py keep_mask).
 * A rank that owns elements [offset, offset + n) of the global batch passes its offset: N ranks draw the masks of a
 * single-process run. Consumed by mla_bn_apply (keep_mask argument). */
int mla_dropout_mask(uint8_t* mask, int64_t n, uint64_t seed, uint64_t stream_id, uint64_t offset, float p_drop,
                     mla_stream_t stream);
/* The same mask with stream_id = stream_base + *counter_dev + 1 read on the device: inside a HIP graph of the training step
 * every replay draws the next mask of the module's sequence (model.py:213 draws a fresh one per forward). */
int mla_dropout_mask_dev(uint8_t* mask, int64_t n, uint64_t seed, uint64_t stream_base, const int64_t* counter_dev,
                         uint64_t offset, float p_drop, mla_stream_t stream);

/* ------------------------------------------------------------------------------------
 * ResNet-50 v1.5 trunk, cnn_type="resnet" (model.py:128-149, torchvision resnet50 as the reference
 * builds it). Activations NHWC in MLA_F32 or MLA_BF16, accumulation f32; images exactly 224 x 224.
 * ---------------------------------------------------------------------------------- */

/* Conv2d weight OIHW f32 (cout, cin, ks, ks) -> [cout][ks][ks][cin] in `dtype` (the layout mla_rn_conv reads): the
 * weights of the convs torchvision's resnet50 builds at model.py:129 (loaded through load_model, train.py:278-281). */
int mla_rn_repack(const float* w_oihw, int64_t cout, int64_t cin, int64_t ks, void* out, int dtype, mla_stream_t stream);

/* Input.forward (model.py:84-101) + resnet.conv1 (7x7 stride 2 pad 3, 3 -> 64, no bias; model.py:129): x (n, H, W) f32
 * planes with H = W = 224 (S_RESNET_SHAPE, params.py:23; anything else is MLA_E_SHAPE); single = 0
 * "repeat" (x in all three channels), 1 "single" (x in channel 0, zeros in 1-2); channels normalised with the ImageNet
 * mean/std, zero padding applied to the NORMALISED channels (a tap outside the image adds nothing). w (64, 3, 7, 7) f32.
 * out NHWC (n, 112, 112, 64) in dtype; scale/shift (64 each, or NULL for the raw conv) then ReLU if relu != 0. */
int mla_rn_stem(const float* x, int64_t n, int64_t H, int64_t W, int single, const float* w, const float* scale, const float* shift, int relu,
                void* out, int dtype, mla_stream_t stream);

/* Bottleneck convs of resnet.layer1..layer4 (model.py:129, applied by CNN.forward at model.py:172-173; conv1x1 / conv3x3 /
 * downsample, bias=False): NHWC in (n, H, W, cin) -> out (n, Ho, Wo, cout)
 * with ks 1 or 3, pad ks/2, stride 1 or 2; cin and cout multiples of 64. w_packed from mla_rn_repack in the same dtype.
 * Epilogue: v = acc; if scale: v = v * scale[c] + shift[c] (eval BatchNorm2d); if residual (same shape as out): v += r;
 * if relu: v = max(v, 0). Deterministic: an output element's reduction order does not depend on n. */
int mla_rn_conv(const void* in, int64_t n, int64_t H, int64_t W, int64_t cin, const void* w_packed, int64_t cout, int64_t ks,
                int64_t stride, const float* scale, const float* shift, const void* residual, int relu, void* out, int dtype,
                mla_stream_t stream);

/* BatchNorm2d in train mode (bn1..bn3 / downsample.1 of model.py:129; the frozen trunk stays in train mode, model.py:132
 * + train.py:111 clf.train()): batch statistics of x (rows = n*H*W, channels),
 * NHWC, channels a multiple of 64. Writes scale = gamma / sqrt(var_b + eps) and shift = beta - mean * scale (for
 * mla_rn_bn_apply), optionally mean / var_biased (NULL to skip), and updates running_mean / running_var (unbiased variance,
 * count = rows; NULL to skip). Sums in double with a fixed reduction order: bit-identical runs.
 * workspace: mla_rn_bn_workspace_bytes(channels) bytes. */
int64_t mla_rn_bn_workspace_bytes(int64_t channels);
int mla_rn_bn_stats(const void* x, int64_t rows, int64_t channels, int dtype, void* workspace, const float* gamma,
                    const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* mean,
                    float* var_biased, float* scale, float* shift, mla_stream_t stream);
/* mla_rn_bn_stats in two stages, so that an all-reduce over the data-parallel ranks fits between them (SyncBN of the
 * trunk: the statistics of the global batch). Stage 1 writes sums = [sum x (channels), sum x^2 (channels), rows] in double
 * (2*channels + 1 elements): the row count travels with the message, so ranks may hold different numbers of rows. Stage 2
 * computes mean, biased variance, scale / shift and the running-statistics update (unbiased variance with the count
 * sums[2*channels], which must be > 0) from the sums; NULL conventions as mla_rn_bn_stats. For one rank, stage 1 followed
 * by stage 2 gives the bits of mla_rn_bn_stats (same partial kernel, slices added in the same order, same finishing
 * arithmetic). workspace: mla_rn_bn_workspace_bytes(channels) bytes, consumed by stage 1. */
int mla_rn_bn_sums(const void* x, int64_t rows, int64_t channels, int dtype, void* workspace, double* sums, mla_stream_t stream);
int mla_rn_bn_finish(const double* sums, int64_t channels, const float* gamma, const float* beta, float eps, float momentum,
                     float* running_mean, float* running_var, float* mean, float* var_biased, float* scale, float* shift,
                     mla_stream_t stream);
/* BatchNorm2d in eval mode (model.py:129 under clf.eval(), train.py:113 and :201): scale / shift from the running statistics, for the mla_rn_conv / mla_rn_stem epilogue. */
int mla_rn_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                          float eps, int64_t channels, float* scale, float* shift, mla_stream_t stream);
/* out = x * scale[c] + shift[c] (+ residual) (ReLU if relu), rows x channels NHWC (channels a multiple of 8): the train-mode
 * bn1/bn2/bn3/downsample.1 of a Bottleneck followed by `out += identity; relu(out)`. out may alias x. */
int mla_rn_bn_apply(const void* x, int64_t rows, int64_t channels, const float* scale, const float* shift, const void* residual,
                    int relu, void* out, int dtype, mla_stream_t stream);

/* resnet.maxpool (model.py:129, child 3 of the model.py:142-146 Sequential): MaxPool2d(3, stride 2, padding 1), NHWC (n, H, W, channels) -> (n, (H-1)/2+1, (W-1)/2+1, channels). */
int mla_rn_maxpool(const void* in, int64_t n, int64_t H, int64_t W, int64_t channels, void* out, int dtype, mla_stream_t stream);
/* resnet.avgpool + CnnFlatten (model.py:188): AdaptiveAvgPool2d(1) of NHWC (n, hw, channels) -> f32 (n, channels). */
int mla_rn_avgpool(const void* in, int64_t n, int64_t hw, int64_t channels, float* out, int dtype, mla_stream_t stream);

/* --- backward of the trunk: cnn_trainable / first_cnn_layer_trainable finetuning (model.py:131-136, loss.backward()
 *     train.py:137). Activations and gradients NHWC in MLA_F32 or MLA_BF16 (f32 accumulation), weight gradients f32 OIHW,
 *     written (not accumulated). No float atomics; every reduction runs in a fixed order (bit-identical runs). --- */

/* Conv2d weight OIHW f32 (cout, cin, ks, ks) -> [cin][ks][ks][cout] in `dtype` with the taps flipped: the weights of the
 * data gradient (a stride-1 data gradient is mla_rn_conv on them). */
int mla_rn_repack_dgrad(const float* w_oihw, int64_t cout, int64_t cin, int64_t ks, void* out, int dtype, mla_stream_t stream);
/* Data gradient of a Bottleneck / downsample conv (model.py:129): dy (n, Ho, Wo, cout) and w_dgrad from mla_rn_repack_dgrad ->
 * dx (n, H, W, cin) [+ residual, same shape as dx: the other branch's gradient]. stride 1: H == Ho; stride 2: H == 2 Ho (four
 * parity classes of input pixel, each with its own tap subset; positions no tap reaches receive the residual alone). */
int mla_rn_conv_dgrad(const void* dy, int64_t n, int64_t Ho, int64_t Wo, int64_t cout, const void* w_dgrad, int64_t cin, int64_t ks,
                      int64_t stride, int64_t H, int64_t W, const void* residual, void* dx, int dtype, mla_stream_t stream);
/* Weight gradient dw (cout, cin, ks, ks) f32 of the conv of mla_rn_conv from its input x (n, H, W, cin) and dy (n, Ho, Wo, cout):
 * a GEMM over the n*Ho*Wo output pixels, split into a shape-determined number of ranges whose f32 partials are added in range
 * order. workspace: mla_rn_conv_wgrad_workspace_floats(n, Ho, Wo, cin, cout, ks, dtype) floats. */
int64_t mla_rn_conv_wgrad_workspace_floats(int64_t n, int64_t Ho, int64_t Wo, int64_t cin, int64_t cout, int64_t ks, int dtype);
int mla_rn_conv_wgrad(const void* x, const void* dy, int64_t n, int64_t H, int64_t W, int64_t cin, int64_t cout, int64_t ks,
                      int64_t stride, float* workspace, int64_t workspace_floats, float* dw_oihw, int dtype, mla_stream_t stream);
/* Weight gradient of the stem (Input.forward model.py:84-101 + resnet.conv1): dw (64, 3, 7, 7) f32 from the raw planes x (n, 224, 224)
 * f32 and dy (n, 112, 112, 64) in dtype. The normalisation is folded in: per (o, tap) S1 = sum dy x and S0 = sum dy over the
 * taps inside the image, dw[o][c][tap] = inv_c ([c carries x] S1 - mean_c S0) (single: x in channel 0 only).
 * workspace: mla_rn_stem_wgrad_workspace_floats(n) floats. */
int64_t mla_rn_stem_wgrad_workspace_floats(int64_t n);
int mla_rn_stem_wgrad(const float* x, int64_t n, int single, const void* dy, float* workspace, int64_t workspace_floats, float* dw,
                      int dtype, mla_stream_t stream);
/* BatchNorm2d train-mode backward (bn1..bn3 / downsample.1 / resnet.bn1): x = the BatchNorm input (raw conv output), mean /
 * var_biased its batch statistics (mla_rn_bn_stats), g = dy masked by y > 0 when y (the kept ReLU output) is non-NULL.
 * dx = gamma invstd (g - mean(g) - xhat mean(g xhat)); dres (or NULL) receives g itself (the residual-path gradient of
 * `relu(bn3 + identity)`); dgamma = sum g xhat, dbeta = sum g (each NULL to skip). Sums in double in the row-slice order
 * of the statistics kernels. workspace: mla_rn_bn_bwd_workspace_bytes(channels) bytes. */
int64_t mla_rn_bn_bwd_workspace_bytes(int64_t channels);
int mla_rn_bn_bwd(const void* x, const void* dy, const void* y, int64_t rows, int64_t channels, const float* mean, const float* var_biased,
                  const float* gamma, float eps, void* workspace, float* dgamma, float* dbeta, void* dx, void* dres, int dtype,
                  mla_stream_t stream);
/* mla_rn_bn_bwd in two stages, so that an all-reduce over the data-parallel ranks fits between them: the backward of the
 * trunk's SyncBN (bn1..bn3 / downsample.1 / resnet.bn1 of model.py:129 under loss.backward(), train.py:137, on the GLOBAL
 * batch). mean / var_biased are the statistics the forward normalised with (under SyncBN those of the global batch,
 * mla_rn_bn_finish). Stage 1 runs the sums of mla_rn_bn_bwd (same kernels, same ReLU mask from y, slices added in the same
 * order) on this rank's rows and writes sums = [sum g (channels), sum g xhat (channels), rows] in double (2*channels + 1
 * elements): the row count travels with the message, so ranks may hold different numbers of rows. dgamma / dbeta (each NULL
 * to skip) are written by STAGE 1 from the LOCAL sums: they are this rank's part of a parameter gradient, which the gradient
 * all-reduce adds over the ranks (taken from the all-reduced sums they would be counted once per rank). Stage 2 forms
 * mean(g) = sums[c] / sums[2*channels] and mean(g xhat) likewise -- the count is read from the message on the device and must
 * be > 0 (it is whenever every contribution came from stage 1, which refuses rows <= 0); the host cannot see it without a
 * blocking copy, so a count that is not > 0 is not MLA_E_ARG but makes every element of dx NaN -- and applies them to this rank's
 * `rows` rows: dx, and dres (or NULL) as in mla_rn_bn_bwd. For one rank, stage 1 followed by stage 2 gives the bits of
 * mla_rn_bn_bwd (same partial and apply kernels, the same per-channel arithmetic). workspace:
 * mla_rn_bn_bwd_workspace_bytes(channels) bytes for either stage; nothing in it has to survive from stage 1 to stage 2
 * (stage 2 holds its per-channel coefficients there). No float atomics; every reduction runs in a fixed order. */
int mla_rn_bn_bwd_sums(const void* x, const void* dy, const void* y, int64_t rows, int64_t channels, const float* mean,
                       const float* var_biased, float eps, void* workspace, double* sums, float* dgamma, float* dbeta, int dtype,
                       mla_stream_t stream);
int mla_rn_bn_bwd_apply(const void* x, const void* dy, const void* y, int64_t rows, int64_t channels, const float* mean,
                        const float* var_biased, const float* gamma, float eps, const double* sums, void* workspace, void* dx, void* dres,
                        int dtype, mla_stream_t stream);
/* Backward of mla_rn_maxpool (resnet.maxpool, model.py:129): in (n, H, W, channels) the pooled input, dy the pooled gradient ->
 * dx (n, H, W, channels). Gradient routed to the FIRST maximum of each window in torch's scan order (ky-major, strict >). */
int mla_rn_maxpool_bwd(const void* in, const void* dy, int64_t n, int64_t H, int64_t W, int64_t channels, void* dx, int dtype,
                       mla_stream_t stream);
/* Backward of mla_rn_avgpool (resnet.avgpool + CnnFlatten, model.py:188): d (n, channels) f32 -> dx (n, hw, channels) = d / hw. */
int mla_rn_avgpool_bwd(const float* d, int64_t n, int64_t hw, int64_t channels, void* dx, int dtype, mla_stream_t stream);

/* --- input gradient of the EVAL-mode trunk (saliency maps of the ResNet branch): under clf.eval() (train.py:113, :201) every
 *     BatchNorm2d of model.py:129 is a per-channel constant folded into the conv epilogue, so its backward is a mask and a
 *     scale; the conv data gradients are mla_rn_conv_dgrad, the pools mla_rn_maxpool_bwd / mla_rn_avgpool_bwd. --- */

/* Backward of the eval epilogue y = [relu](conv * scale[c] + shift[c] [+ residual]) over NHWC rows x channels (channels a
 * multiple of 8), dy / y / dpre / dres in dtype: g = dy * (y > 0), or dy itself when y is NULL (no ReLU: downsample.1); NaN in y
 * gives 0, as torch's threshold_backward. dpre = g * scale[c], the gradient of the conv output: in f32 the product as written,
 * in bf16 the same f32 value rounded once. dres (or NULL) receives g, the gradient of the residual. */
int mla_rn_act_bwd(const void* dy, const void* y, const float* scale, int64_t rows, int64_t channels, void* dpre, void* dres, int dtype,
                   mla_stream_t stream);
/* Data gradient of the stem (Input.forward model.py:84-101 + resnet.conv1, 7x7 stride 2 pad 3) with respect to the RAW planes:
 * dy (n, 112, 112, 64) in dtype, w (64, 3, 7, 7) f32 -> dx (n, 224, 224) f32, every element written once (nothing to zero, no
 * workspace, no atomics; the bits do not depend on n). The channel configuration (single: x in channel 0 only, else repeated) and
 * the three 1 / std_c are folded into the taps as mla_rn_stem folds them. y (n, 112, 112, 64) in dtype with scale[64], both or
 * neither: the stem's fused eval output and its BatchNorm scale; then the gradient that enters the conv is dy * (y > 0) * scale[o]
 * (NaN in y gives 0). dy and y 16-byte aligned. */
int mla_rn_stem_dgrad(const void* dy, int64_t n, const void* y, const float* scale, const float* w, int single, float* dx, int dtype,
                      mla_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MLA_HIP_H */
