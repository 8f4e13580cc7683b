"""Drop-in for the hot-path-adjacent part of the reference's ``dataset.py``:
the native spectrogram path of ``create_spec`` (dataset.py:318-324) and ``split`` /
``overlapping_split`` / ``contiguous_split`` (dataset.py:329-363), i.e. the actual caller of
``waveform_to_examples`` in the reference's data pipeline. Same names and argument order; tensors
stay on the GPU. The ResNet variant of the librosa path (dataset.py:308-316: melspectrogram + power_to_db with librosa's
defaults) runs on the HIP kernels of csrc/melspec.hip, and so does the VGGish variant of the librosa path (dataset.py:305-307:
HTK basis, center=False) through the ``*_librosa`` functions at the end of this file; the UrbanSound8K fold logic and the HDF5
writer are outside scope.

``clips_to_frames`` is the batched fast path: PCM of many clips -> (clips, T, 1, 64, 96) in two
kernels (fused log-mel + the re-framing gather), which is the tensor ``Input`` reshapes at
model.py:98-99 (a reshape, not a transpose -- reproduced as is). ``clips_to_images`` is the same for the ResNet branch:
PCM of many clips -> (clips, T, 1, 224, 224) in two kernels (mel-dB spectrogram + clip-and-split gather)."""

import ctypes
import struct

import numpy as np
import torch

from . import _lib, frontend
from .params import S_RESNET_SHAPE, SAMPLES_NUM_RESNET, SR_RESNET, T


def _frames(examples, clips, ex_per_clip, n_frames, frame_len, stride):
    out = torch.empty((clips, n_frames, 64, frame_len), dtype=torch.float32, device=examples.device)
    vp = ctypes.c_void_p
    _lib.check(_lib.lib().mla_dataset_frames(vp(examples.data_ptr()), clips, ex_per_clip, n_frames, frame_len, stride,
                                             vp(out.data_ptr()), _lib.stream_ptr()))
    return out


def create_spec(audio_array, cnn_type, sr, samples_num, x_size, y_size, use_librosa, overlap):
    """Spectrogram of one clip on the GPU: (64, 384) for the native VGGish path, (y_size, 1 + n // hop) dB values for
    cnn_type="resnet" (always the librosa path: load_hdf5 forces use_librosa for it, dataset.py:176-178)."""
    if cnn_type == "resnet":
        hop = resnet_hop_length(samples_num, x_size, overlap)
        return frontend.melspectrogram_db(frontend.as_device_mono(audio_array)[None], sr, y_size, hop)[0]
    if use_librosa or cnn_type != "vggish":
        raise NotImplementedError("create_spec builds cnn_type='resnet' (always the librosa path) and the native VGGish path "
                                  "(use_librosa=False); the VGGish librosa path (HTK mel-dB, center=False) is create_spec_librosa")
    ex = frontend.waveforms_to_examples(frontend.as_device_mono(audio_array)[None])
    if ex.shape[0] > 4:
        raise ValueError("could not broadcast input array from shape (%d,96,64) into shape (4,96,64)" % ex.shape[0])
    return _frames(ex, 1, ex.shape[0], 1, 384, 0)[0, 0]


def resnet_hop_length(samples_num, x_size, overlap):
    """dataset.py:309-311: four image widths of columns per clip when the images overlap, T widths when they do not."""
    return samples_num // (x_size * 4) if overlap else samples_num // (x_size * T)


def overlapping_split(spec, num_frames, frame_length):
    """Zero-copy strided view (num_frames, 64, frame_length), stride (W - frame_length) // (num_frames - 1)."""
    stride = (spec.shape[1] - frame_length) // (num_frames - 1)
    return spec.unfold(1, frame_length, stride).permute(1, 0, 2)[:num_frames]


def contiguous_split(spec, num_frames, frame_length):
    return spec.unfold(1, frame_length, frame_length).permute(1, 0, 2)[:num_frames]


def split(spec, num_frames, x_size, y_size, overlap):
    frames = overlapping_split(spec, num_frames, x_size) if overlap else contiguous_split(spec, num_frames, x_size)
    assert tuple(frames.shape[1:]) == (y_size, x_size)
    return frames


def clips_to_frames(pcm, overlap=True):
    """(clips, n_samples) device PCM (<= 4 s per clip) -> (clips, T, 1, 64, 96) float32, the layout
    load_hdf5 stores (dataset.py:252-255) and Ensemble consumes."""
    clips = pcm.shape[0]
    ex = frontend.waveforms_to_examples(pcm)
    per = ex.shape[0] // max(clips, 1)
    if per > 4:
        raise ValueError("clips longer than 4 examples do not fit the 4-slot spectrogram (dataset.py:321-322)")
    n = T if overlap else 4
    stride = (384 - 96) // (T - 1) if overlap else 96
    return _frames(ex, clips, per, n, 96, stride)[:, :, None]


def clips_to_images(pcm, overlap=True):
    """(clips, SAMPLES_NUM_RESNET) float32 device PCM at SR_RESNET -> (clips, T, 1, 224, 224) float32, the tensor load_hdf5
    stores for cnn_type="resnet" (dataset.py:243-254) and Ensemble consumes; bit-identical to create_spec + split per clip.
    Rows are exactly SAMPLES_NUM_RESNET samples: the caller cuts longer clips and zero-fills shorter ones, as load_hdf5 means to."""
    pcm = _resnet_rows(pcm, "clips_to_images")
    hop, step = _image_geometry(overlap)
    db, ws = frontend.melspec_db_unclipped(pcm, SR_RESNET, S_RESNET_SHAPE[0], hop)
    return frontend.melspec_images(db, ws, SAMPLES_NUM_RESNET, hop, 80.0, T, S_RESNET_SHAPE[1], step)


def _resnet_rows(pcm, what):
    assert pcm.dim() == 2 and pcm.is_cuda
    if pcm.shape[1] != SAMPLES_NUM_RESNET:
        raise ValueError("%s takes rows of exactly %d samples (%d s at %d Hz), got %d"
                         % (what, SAMPLES_NUM_RESNET, SAMPLES_NUM_RESNET // SR_RESNET, SR_RESNET, pcm.shape[1]))
    return pcm if pcm.dtype == torch.float32 else pcm.float()


def _image_geometry(overlap):
    """(hop length, columns between the starts of two images) of clips_to_images."""
    x_size = S_RESNET_SHAPE[1]
    hop = resnet_hop_length(SAMPLES_NUM_RESNET, x_size, overlap)
    width = frontend.melspec_frames(SAMPLES_NUM_RESNET, hop)
    return hop, (width - x_size) // (T - 1) if overlap else x_size


def clips_to_images_backward(pcm, grad_images, overlap=True, floor_grad=True):
    """The gradient of ``clips_to_images(pcm, overlap)`` with respect to the waveform: (clips, SAMPLES_NUM_RESNET) float32 device PCM
    and grad_images (clips, T, 1, 224, 224) float32 -> (clips, SAMPLES_NUM_RESNET) float32. The spectrogram and its maxima are
    computed again (the forward's first launch, same bits), then the two launches of csrc/melspec_bwd.hip:
    frontend.melspec_images_backward (which explains floor_grad) and frontend.melspec_db_backward. float32 whatever the model's
    precision; deterministic, and a clip's gradient does not depend on the batch."""
    pcm = _resnet_rows(pcm, "clips_to_images_backward")
    hop, step = _image_geometry(overlap)
    y_size, x_size = S_RESNET_SHAPE
    db, ws = frontend.melspec_db_unclipped(pcm, SR_RESNET, y_size, hop)
    d_db = frontend.melspec_images_backward(grad_images.float(), db, ws, SAMPLES_NUM_RESNET, hop, 80.0, T, x_size, step, floor_grad)
    return frontend.melspec_db_backward(pcm, d_db, SR_RESNET, y_size, hop)


def clips_to_images_differentiable(pcm, overlap=True):
    """``clips_to_images`` behind autograd: (clips, SAMPLES_NUM_RESNET) float32 device PCM that may require grad -> images attached
    to the graph (differentiable.MelDbImagesFn: the forward is the same two launches and gives the same bits, the backward is the
    two launches of clips_to_images_backward with the floor's own gradient, as torch.autograd would give it)."""
    from . import differentiable
    return differentiable.MelDbImagesFn.apply(pcm, overlap)


def _host_recording(x, index):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.ndim not in (1, 2) or (x.ndim == 2 and x.shape[1] < 1):
        raise ValueError("recording %d: expected (n,) or (n, channels), got shape %r" % (index, tuple(x.shape)))
    if x.dtype != np.int16:
        if not np.issubdtype(x.dtype, np.floating):
            raise TypeError("recording %d: int16 or floating samples expected, got %s" % (index, x.dtype))
        x = x.astype(np.float32, copy=False)               # float64 is rounded once, as frontend.as_device_mono does
    return x


def recordings_to_clips(recordings, rates, sr=SR_RESNET, samples_num=SAMPLES_NUM_RESNET):
    """Recordings as they are decoded -> the (B, samples_num) float32 device tensor clips_to_images and Ensemble.forward_clips
    take: librosa.load(path, sr=sr) (channel mean, resampy 'kaiser_best'; no resampling at an equal rate), the cut at
    samples_num and the zero fill of dataset.py:232-237, for the whole batch in one launch (frontend.prepare_clips).

    recordings: a sequence of host arrays or tensors, each (n,) or (n, channels) with interleaved channels as `wave` and
    `soundfile` deliver them; all int16 (scaled by 1/32768) or all floating. rates: one rate in Hz per recording, or one number.
    The WHOLE recording is resampled and the cut comes afterwards, as in the reference. The samples travel through one packed
    pinned host buffer and one copy, the descriptors through another. ValueError (naming the recording) where resampy raises,
    before anything is copied or launched. An empty sequence gives a (0, samples_num) tensor."""
    recs, rates = _checked_recordings(recordings, rates, sr)
    return _pack_recordings(recs, rates, sr, samples_num)


def _checked_recordings(recordings, rates, sr):
    """recordings_to_clips' checks, all before anything is copied or launched -> (host arrays, one rate per recording)."""
    recs = [_host_recording(x, i) for i, x in enumerate(recordings)]
    B = len(recs)
    rates = [rates] * B if np.isscalar(rates) else list(rates)
    if len(rates) != B:
        raise ValueError("%d recordings but %d rates" % (B, len(rates)))
    if sr <= 0:
        raise ValueError("Invalid sample rate: sr_new=%r" % (sr,))
    if len({x.dtype == np.int16 for x in recs}) > 1:
        raise TypeError("recordings must be all int16 or all floating, not a mixture")
    for i, (x, r) in enumerate(zip(recs, rates)):
        if r <= 0:
            raise ValueError("recording %d: Invalid sample rate: sr_orig=%r" % (i, r))
        _check_resamples(i, x.shape[0], r, sr)
    return recs, rates


def _check_resamples(index, frames, rate, sr):
    """resampy's refusal of an input whose resampled length is zero (a recording at `sr` already is not resampled)."""
    if float(rate) != float(sr) and int(frames * (float(sr) / float(rate))) < 1:
        raise ValueError("recording %d: Input signal length=%d is too small to resample from %s->%s" % (index, frames, rate, sr))


def _packed_on_device(chunks, dtype, align=1):
    """1-D host arrays -> (one device tensor holding them back to back, each starting on a multiple of `align` elements, the
    element offset of each): one pinned buffer, one copy."""
    dev = frontend._device()                                # no GPU: refused before any pinned memory is asked for
    sizes = np.array([c.shape[0] for c in chunks], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum((sizes + align - 1) // align * align)[:-1]]).astype(np.int64)
    host = torch.empty(int(offsets[-1] + sizes[-1]), dtype=dtype, pin_memory=True)
    flat = host.numpy()
    for c, o, s in zip(chunks, offsets, sizes):
        flat[o:o + s] = c
    return host.to(dev, non_blocking=True), offsets


def _pack_recordings(recs, rates, sr, samples_num):
    if not recs:
        return torch.empty((0, int(samples_num)), dtype=torch.float32, device="cuda" if torch.cuda.is_available() else "cpu")
    frames = np.array([x.shape[0] for x in recs], dtype=np.int64)
    channels = np.array([1 if x.ndim == 1 else x.shape[1] for x in recs], dtype=np.int32)
    packed, offsets = _packed_on_device([x.reshape(-1) for x in recs], torch.int16 if recs[0].dtype == np.int16 else torch.float32)
    return frontend.prepare_clips(packed, offsets, frames, channels, np.array(rates, dtype=np.float64), sr, samples_num)


def read_wav16(path):
    """16-bit RIFF file -> ((frames,) or (frames, channels) int16 array, rate), with the stdlib `wave` module and the refusal of
    vggish_input.wavfile_to_examples for any other sample width."""
    import wave
    with wave.open(path, "rb") as wf:
        assert wf.getsampwidth() == 2, "Bad sample type: %r" % wf.getsampwidth()
        sr, ch = wf.getframerate(), wf.getnchannels()
        pcm = np.frombuffer(wf.readframes(wf.getnframes()), dtype=np.int16)
    return (pcm.reshape(-1, ch) if ch > 1 else pcm), sr


def _read_wav16s(paths):
    """read_wav16 on every path -> (recordings, rates)."""
    decoded = [read_wav16(str(p)) for p in paths]
    return [d[0] for d in decoded], [d[1] for d in decoded]


def wavfiles_to_clips(paths, sr=SR_RESNET, samples_num=SAMPLES_NUM_RESNET):
    """16-bit WAV files -> (B, samples_num) clips: read_wav16 on every path, then recordings_to_clips."""
    return recordings_to_clips(*_read_wav16s(paths), sr, samples_num)


# WAVE format tags read_audiofile refuses by name (everything but PCM, IEEE float and their extensible form is refused)
_WAVE_TAGS = {0x0002: "MS ADPCM", 0x0006: "A-law", 0x0007: "mu-law", 0x0011: "IMA ADPCM", 0x0055: "MP3"}
_PCM_FORMATS = {8: _lib.U8, 16: _lib.I16, 24: _lib.I24, 32: _lib.I32}
_FLOAT_FORMATS = {32: _lib.F32, 64: _lib.F64}


def read_audiofile(path):
    """RIFF/WAVE file -> (the data chunk's bytes as a 1-D uint8 array, (format code, channels, rate, frames)), without converting
    a sample: what librosa.load reads through libsndfile (dataset.py:232 of the reference) for PCM of 8, 16, 24 or 32 bits and
    IEEE float of 32 or 64 bits, plain or WAVE_FORMAT_EXTENSIBLE (the container width counts: samples are left-justified). The
    format code is _lib.U8 / I16 / I24 / I32 / F32 / F64, as frontend.prepare_clips_raw takes it. Chunks are walked in file
    order (word-aligned; unknown ones are skipped). frames = min(declared data size, bytes present) // block align: a truncated
    file or a trailing partial frame loses the incomplete part only, as with libsndfile. ValueError, naming the path, for
    anything else: no RIFF/WAVE header (RIFX and RF64 included), no `fmt ` before `data`, no `data`, another tag or width, zero
    channels or rate, a block align that is not channels * bits / 8."""
    path = str(path)
    with open(path, "rb") as f:
        raw = f.read()

    def bad(reason):
        return ValueError("%s: %s" % (path, reason))

    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        raise bad("not a RIFF/WAVE file (header %r)" % (raw[:4] + raw[8:12],))
    fmt, pos = None, 12
    while pos + 8 <= len(raw):
        cid, size = struct.unpack_from("<4sI", raw, pos)
        pos += 8
        if cid == b"fmt ":
            if size < 16 or pos + size > len(raw):
                raise bad("fmt chunk of %d bytes is too short" % min(size, len(raw) - pos))
            tag, ch, rate, _, align, bits = struct.unpack_from("<HHIIHH", raw, pos)
            if tag == 0xFFFE:
                if size < 40:
                    raise bad("extensible fmt chunk of %d bytes is too short" % size)
                tag = struct.unpack_from("<H", raw, pos + 24)[0]             # first two bytes of the sub-format GUID
            if tag not in (1, 3):
                raise bad("format tag 0x%04x (%s) is not supported: PCM or IEEE float only" % (tag, _WAVE_TAGS.get(tag, "unknown")))
            code = (_PCM_FORMATS if tag == 1 else _FLOAT_FORMATS).get(bits)
            if code is None:
                raise bad("%d-bit %s samples are not supported" % (bits, "PCM" if tag == 1 else "float"))
            if ch < 1:
                raise bad("zero channels")
            if rate < 1:
                raise bad("a rate of zero")
            if align != ch * bits // 8:
                raise bad("block align %d is not %d channels * %d bits / 8" % (align, ch, bits))
            fmt = (code, ch, rate, align)
        elif cid == b"data":
            if fmt is None:
                raise bad("no fmt chunk before the data chunk")
            code, ch, rate, align = fmt
            frames = min(size, len(raw) - pos) // align
            return np.frombuffer(raw, dtype=np.uint8, count=frames * align, offset=pos), (code, ch, rate, frames)
        pos += size + (size & 1)
    raise bad("no data chunk")


_SAMPLE_DTYPES = {_lib.U8: "u1", _lib.I16: "<i2", _lib.I32: "<i4", _lib.F32: "<f4", _lib.F64: "<f8"}


def decode_audiofile(path):
    """RIFF/WAVE file -> ((frames,) or (frames, channels) float32 array, rate): read_audiofile's bytes decoded on the host with
    numpy, PCM scaled to [-1, 1) (8-bit: (x - 128) / 128; n-bit: x / 2**(n - 1)), float64 rounded to float32 -- what
    soundfile.read(path, dtype="float32") returns. For callers who want arrays; the batched path decodes on the device."""
    data, (code, ch, rate, frames) = read_audiofile(path)
    if code == _lib.I24:
        b = data.reshape(-1, 3).astype(np.int32)
        x = ((b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16) << 8 >> 8).astype(np.float32) / np.float32(8388608.0)
    else:
        x = data.view(_SAMPLE_DTYPES[code])
        if code == _lib.U8:
            x = (x.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
        elif code == _lib.I16:
            x = x.astype(np.float32) / np.float32(32768.0)
        elif code == _lib.I32:
            x = (x.astype(np.float64) / 2147483648.0).astype(np.float32)          # one rounding per sample
        else:
            x = x.astype(np.float32)
    return (x.reshape(frames, ch) if ch > 1 else x), rate


def audiofiles_to_clips(paths, sr=SR_RESNET, samples_num=SAMPLES_NUM_RESNET):
    """WAV files of any mixture of encodings read_audiofile accepts -> (B, samples_num) clips, as recordings_to_clips makes them:
    the data chunks go back to back (each on a multiple of 8 bytes) into one pinned byte buffer as they sit in the files, travel
    in one copy and are decoded, mixed, resampled, cut and zero-filled in one launch (frontend.prepare_clips_raw). The first
    unreadable file raises, naming it; the checks and messages of recordings_to_clips come before anything is copied."""
    return _pack_audiofiles(_checked_audiofiles(paths, sr), sr, samples_num)


def _checked_audiofiles(paths, sr):
    files = [read_audiofile(p) for p in paths]
    if sr <= 0:
        raise ValueError("Invalid sample rate: sr_new=%r" % (sr,))
    for i, (_, (_, _, r, n)) in enumerate(files):
        _check_resamples(i, n, r, sr)
    return files


def _pack_audiofiles(files, sr, samples_num):
    if not files:
        return torch.empty((0, int(samples_num)), dtype=torch.float32, device="cuda" if torch.cuda.is_available() else "cpu")
    packed, offsets = _packed_on_device([d for d, _ in files], torch.uint8, align=8)
    code, ch, rate, frames = zip(*(desc for _, desc in files))
    return frontend.prepare_clips_raw(packed, offsets, np.array(frames, dtype=np.int64), np.array(ch, dtype=np.int32),
                                      np.array(rate, dtype=np.float64), np.array(code, dtype=np.int32), sr, samples_num)


# ---- the VGGish branch from recordings: load_hdf5(cnn_type="vggish", use_librosa=False), dataset.py:239-254 -----------------------
SR_VGGISH = 16000
SAMPLES_NUM_VGGISH = 15600 + 3 * 15360          # 61 680: all that four 0.96 s examples read


def _bag_counts(frames, rates):
    """Whole 0.96 s examples of every recording once it is at 16 kHz: n_res from the library's resampled length (the frames
    themselves at 16 kHz), examples from mla_logmel_counts. ValueError, naming the recording, where the reference raises: fewer
    than 240 samples (mel_features.py:42-45) or more than the 4 slots of create_spec (dataset.py:321-322)."""
    L = _lib.lib()
    counts = np.zeros(len(frames), dtype=np.int32)
    for i, (n, r) in enumerate(zip(frames, rates)):
        n_res = int(n) if float(r) == float(SR_VGGISH) else int(L.mla_resample_length(int(n), float(r), float(SR_VGGISH)))
        try:
            counts[i] = frontend.counts(n_res)[1]
        except ValueError as e:
            raise ValueError("recording %d: %s (%d samples at 16 kHz)" % (i, e, n_res)) from None
        if counts[i] > 4:
            raise ValueError("recording %d: could not broadcast input array from shape (%d,96,64) into shape (4,96,64)" % (i, counts[i]))
    return counts


def _bags(clips, counts, overlap, out_dtype):
    n = T if overlap else 4
    if clips.shape[0] == 0:
        return torch.empty((0, n, 1, 64, 96), dtype=out_dtype, device=clips.device)
    return frontend.logmel_bags(clips, counts, n, (384 - 96) // (T - 1) if overlap else 96, out_dtype)


def recordings_to_frames(recordings, rates, overlap=True, out_dtype=torch.float32):
    """Recordings as they are decoded -> the (B, T, 1, 64, 96) bag tensor load_hdf5(cnn_type="vggish", use_librosa=False) stores
    (dataset.py:239-254) and Ensemble consumes, in TWO launches whatever B is: recordings_to_clips at 16 kHz (channel mean, resampy
    'kaiser_best' resampling of the whole recording) into rows of 61 680 samples, then frontend.logmel_bags with the number of
    whole 0.96 s examples of each recording. As in the reference the waveform is not zero-filled: a trailing partial example is
    dropped and the slots a recording lacks are 0.0 (a recording shorter than 0.975 s gives an all-zero bag). overlap=False gives
    4 frames per bag (contiguous_split). out_dtype: torch.float32 or torch.bfloat16 (one rounding of the float32 value).
    recordings / rates: as recordings_to_clips takes them, with its errors; further ValueErrors, naming the recording, where the
    reference raises: fewer than 240 samples at 16 kHz ("negative dimensions are not allowed") and more than 4 examples
    (77 040 samples or more). All of them come before anything is copied or launched. An empty sequence gives (0, T, 1, 64, 96)."""
    recs, rates = _checked_recordings(recordings, rates, SR_VGGISH)
    counts = _bag_counts([x.shape[0] for x in recs], rates)
    return _bags(_pack_recordings(recs, rates, SR_VGGISH, SAMPLES_NUM_VGGISH), counts, overlap, out_dtype)


def wavfiles_to_frames(paths, overlap=True, out_dtype=torch.float32):
    """16-bit WAV files -> (B, T, 1, 64, 96) bags: read_wav16 on every path (other widths are refused), then recordings_to_frames."""
    return recordings_to_frames(*_read_wav16s(paths), overlap, out_dtype)


def audiofiles_to_frames(paths, overlap=True, out_dtype=torch.float32):
    """WAV files of any mixture of encodings read_audiofile accepts -> (B, T, 1, 64, 96) bags, in two launches: the files' bytes
    are decoded, mixed and resampled to 16 kHz by frontend.prepare_clips_raw, then frontend.logmel_bags. Bit-identical to
    wavfiles_to_frames for 16-bit files; other encodings are decoded at full precision (the reference's sf.read(dtype="int16")
    quantises them to int16 first: DESIGN.md section 7)."""
    files = _checked_audiofiles(paths, SR_VGGISH)
    counts = _bag_counts([d[1][3] for d in files], [d[1][2] for d in files])
    return _bags(_pack_audiofiles(files, SR_VGGISH, SAMPLES_NUM_VGGISH), counts, overlap, out_dtype)


# ---- timelines: recordings of any length in windows of four examples (no counterpart in the reference, whose loader stops at 4 s) ----
HOP_SECONDS = 0.32                                # one slot of hop: 32 log-mel columns
_CLIPS_MAX_SAMPLES = 0x7fffffff - 256             # mla_clips_prepare: samples_num, and rows * ceil(samples_num / 256) workgroups


def timeline_counts(n, hop_slots=3):
    """(windows, kept slots, samples read) of a recording of n samples at 16 kHz scored at a hop of hop_slots * 0.32 s:
    frontend.timeline_counts. n >= 61 680: windows = 1 + (n - 61 680) // (5 120 * hop_slots), window j the native bag of
    wave[5 120 * hop_slots * j :][: 61 680]; 240 <= n < 61 680: one window, the bag recordings_to_frames gives; n < 240: ValueError."""
    return frontend.timeline_counts(n, hop_slots)


def _timeline_lengths(frames, rates, hop_slots):
    """Samples of every recording once it is at 16 kHz (the library's resampled length), checked: ValueError, naming the recording,
    for fewer than 240 of them; and for a batch whose rows the clips launch cannot tile. -> (lengths, samples per row)."""
    if int(hop_slots) != hop_slots or hop_slots < 1:
        raise ValueError("hop_slots must be an integer >= 1 (the hop is hop_slots * 0.32 s), got %r" % (hop_slots,))
    L = _lib.lib()
    n16, most = np.zeros(len(frames), dtype=np.int64), 1
    for i, (n, r) in enumerate(zip(frames, rates)):
        n16[i] = int(n) if float(r) == float(SR_VGGISH) else int(L.mla_resample_length(int(n), float(r), float(SR_VGGISH)))
        try:
            most = max(most, frontend.timeline_counts(n16[i], hop_slots)[2])
        except ValueError as e:
            raise ValueError("recording %d: %s (%d samples at 16 kHz)" % (i, e, n16[i])) from None
    if most > _CLIPS_MAX_SAMPLES or len(frames) * ((most + 255) // 256) > 0x7fffffff:
        raise ValueError("%d recordings of up to %d samples at 16 kHz are more than one clips launch tiles (rows of at most %d "
                         "samples, at most 2**31 - 1 tiles of 256 samples in the batch): split the batch" % (len(frames), most, _CLIPS_MAX_SAMPLES))
    return n16, most


def _slots(clips, n16, hop_slots, out_dtype):
    if clips.shape[0] == 0:
        none = np.zeros(0, dtype=np.int64)
        return torch.empty((0, 64, 96), dtype=out_dtype, device=clips.device), none, none, np.zeros(0, dtype=np.float64)
    slots, first_rows, index = frontend.logmel_timeline(clips, n16, hop_slots, out_dtype)
    step = min(int(hop_slots), T)
    starts = np.zeros(first_rows.shape[0], dtype=np.float64)
    if first_rows.shape[0]:
        first = first_rows[np.searchsorted(index, index)]          # the first window's row of each window's recording
        starts = HOP_SECONDS * hop_slots * ((first_rows - first) // step)
    return slots, first_rows, index, starts


def recordings_to_slots(recordings, rates, hop_slots=3, out_dtype=torch.float32):
    """Recordings of ANY length as they are decoded -> (slots, first_rows, recording_index, start_seconds) in TWO launches
    whatever the batch is: recordings_to_clips at 16 kHz (channel mean, resampy 'kaiser_best' over the whole recording) into rows
    as long as the longest recording needs, then frontend.logmel_timeline.

    A recording of n samples at 16 kHz is scored in windows of four 0.96 s examples (61 680 samples, the bag of
    recordings_to_frames) that start hop_slots * 0.32 s apart: timeline_counts(n, hop_slots). A trailing stretch that fills no
    window is dropped, as the reference drops a trailing partial example; a recording shorter than one window gives the one bag
    recordings_to_frames gives. slots: (S, 64, 96) device tensor in out_dtype (float32, or bfloat16 with one rounding), the
    distinct 96-column slots of all windows, each computed once; first_rows / recording_index (host int64) and start_seconds (host
    float64) have one entry per window: slots[first_rows[w] : first_rows[w] + 10] is the (10, 64, 96) bag of the window that starts
    start_seconds[w] into recordings[recording_index[w]], bit for bit the bag recordings_to_frames gives for that crop of the
    resampled recording. recordings / rates: as recordings_to_clips takes them, with its errors; ValueError, naming the recording,
    for fewer than 240 samples at 16 kHz. Limit (the clips launch tiles a row in 256-sample workgroups): rows of at most
    2**31 - 257 samples, about 37 hours, and at most 2**31 - 1 tiles in the batch; more raises ValueError. All errors come before
    anything is copied or launched."""
    recs, rates = _checked_recordings(recordings, rates, SR_VGGISH)
    n16, most = _timeline_lengths([x.shape[0] for x in recs], rates, hop_slots)
    return _slots(_pack_recordings(recs, rates, SR_VGGISH, most), n16, hop_slots, out_dtype)


def wavfiles_to_slots(paths, hop_slots=3, out_dtype=torch.float32):
    """16-bit WAV files -> recordings_to_slots: read_wav16 on every path (other widths are refused)."""
    return recordings_to_slots(*_read_wav16s(paths), hop_slots, out_dtype)


def audiofiles_to_slots(paths, hop_slots=3, out_dtype=torch.float32):
    """WAV files of any mixture of encodings read_audiofile accepts -> what recordings_to_slots returns, in two launches: the
    files' bytes are decoded, mixed and resampled to 16 kHz by frontend.prepare_clips_raw, then frontend.logmel_timeline.
    Bit-identical to wavfiles_to_slots for 16-bit files."""
    files = _checked_audiofiles(paths, SR_VGGISH)
    n16, most = _timeline_lengths([d[1][3] for d in files], [d[1][2] for d in files], hop_slots)
    return _slots(_pack_audiofiles(files, SR_VGGISH, most), n16, hop_slots, out_dtype)


# ---- image timelines: the ResNet branch over recordings of any length (no counterpart in the reference, whose loader stops at 4 s) ----
IMAGE_HOP_SECONDS = 1.0 / 3                       # one image of hop: 75 spectrogram columns of 98 samples at 22 050 Hz
_TRACK_MAX_SAMPLES = 1 << 30                      # mla_melspec_track_db: a track's padded samples are indexed with int


def image_timeline_counts(n, hop_images=3):
    """(windows, kept images, track samples L, track columns C) of a recording of n samples at 22 050 Hz scored in 4 s windows
    (88 200 samples, the reference's clip) that start hop_images / 3 s apart: frontend.melspec_track_counts. n >= 88 200: windows =
    1 + (n - 88 200) // (7 350 * hop_images), a trailing stretch that fills no window is dropped; n < 88 200: one window, the
    recording zero-filled as forward_recordings does. The track is the first L = 88 200 + 7 350 * hop_images * (windows - 1)
    samples, C = 1 + L // 98 columns."""
    return frontend.melspec_track_counts(n, hop_images)


def _track_lengths(frames, rates, hop_images):
    """Samples of every recording once it is at 22 050 Hz (the library's resampled length), checked: ValueError for a hop_images
    that is no integer >= 1, for a track longer than 2**30 samples (naming the recording) and for a batch whose rows the clips
    launch cannot tile. -> (lengths, samples per row: the longest track)."""
    if int(hop_images) != hop_images or hop_images < 1:
        raise ValueError("hop_images must be an integer >= 1 (the hop is hop_images / 3 s), got %r" % (hop_images,))
    L = _lib.lib()
    n22, most = np.zeros(len(frames), dtype=np.int64), SAMPLES_NUM_RESNET
    for i, (n, r) in enumerate(zip(frames, rates)):
        n22[i] = int(n) if float(r) == float(SR_RESNET) else int(L.mla_resample_length(int(n), float(r), float(SR_RESNET)))
        track = frontend.melspec_track_counts(n22[i], hop_images)[2]
        if track > _TRACK_MAX_SAMPLES:
            raise ValueError("recording %d: a track of %d samples at 22 050 Hz is longer than 2**30 (about 13.5 hours): split the recording"
                             % (i, track))
        most = max(most, track)
    if len(frames) * ((most + 255) // 256) > 0x7fffffff:
        raise ValueError("%d recordings of up to %d samples at 22 050 Hz are more than one clips launch tiles (at most 2**31 - 1 tiles "
                         "of 256 samples in the batch): split the batch" % (len(frames), most))
    return n22, most


def _tracks(clips, n22, hop_images):
    """(the frontend.Track of the batch, start_seconds of every window)."""
    track = frontend.melspec_track_db(clips, n22, hop_images)
    starts = np.zeros(track.first_rows.shape[0], dtype=np.float64)
    if starts.shape[0]:
        index = track.recording_index
        j = np.arange(index.shape[0]) - np.searchsorted(index, index)          # the window's number within its recording
        starts = int(hop_images) * j / 3.0
    return track, starts


def _no_tracks():
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    none = np.zeros(0, dtype=np.int64)
    return torch.empty((0, 1) + S_RESNET_SHAPE, dtype=torch.float32, device=dev), none, none, np.zeros(0, dtype=np.float64)


def recordings_to_tracks(recordings, rates, hop_images=3):
    """Recordings of ANY length as they are decoded -> (frontend.Track, start_seconds) in THREE launches whatever the batch is:
    recordings_to_clips at 22 050 Hz into rows as long as the longest track, then frontend.melspec_track_db's two. The images are
    not made: frontend.melspec_track_images(track, first, count) makes any range of them (Ensemble.score_image_timeline does, chunk
    by chunk). Arguments, errors and limits: recordings_to_track_images. An empty sequence gives (None, no seconds)."""
    recs, rates = _checked_recordings(recordings, rates, SR_RESNET)
    n22, most = _track_lengths([x.shape[0] for x in recs], rates, hop_images)
    if not recs:
        return None, np.zeros(0, dtype=np.float64)
    return _tracks(_pack_recordings(recs, rates, SR_RESNET, most), n22, hop_images)


def wavfiles_to_tracks(paths, hop_images=3):
    """16-bit WAV files -> recordings_to_tracks: read_wav16 on every path (other widths are refused)."""
    return recordings_to_tracks(*_read_wav16s(paths), hop_images)


def audiofiles_to_tracks(paths, hop_images=3):
    """WAV files of any mixture of encodings read_audiofile accepts -> what recordings_to_tracks returns: the files' bytes are decoded,
    mixed and resampled to 22 050 Hz by frontend.prepare_clips_raw. Bit-identical to wavfiles_to_tracks for 16-bit files."""
    files = _checked_audiofiles(paths, SR_RESNET)
    n22, most = _track_lengths([d[1][3] for d in files], [d[1][2] for d in files], hop_images)
    if not files:
        return None, np.zeros(0, dtype=np.float64)
    return _tracks(_pack_audiofiles(files, SR_RESNET, most), n22, hop_images)


def _track_images(track, starts):
    if track is None:
        return _no_tracks()
    images = frontend.melspec_track_images(track, 0, track.descriptors.images)
    return images, track.first_rows, track.recording_index, starts


def recordings_to_track_images(recordings, rates, hop_images=3):
    """Recordings of ANY length as they are decoded -> (images, first_rows, recording_index, start_seconds) in FOUR launches
    whatever the batch is: recordings_to_clips at 22 050 Hz (channel mean, resampy 'kaiser_best' over the whole recording) into rows
    as long as the longest track, then the track's spectrogram, its maximum and the images (csrc/melspec.hip).

    A recording of n samples at 22 050 Hz is scored in windows of 88 200 samples, the reference's 4 s clip, that start
    hop_images / 3 s apart: image_timeline_counts(n, hop_images). A trailing stretch that fills no window is dropped; a recording
    shorter than one window is zero-filled and gives the ten images forward_recordings builds, bit for bit. images: (S, 1, 224, 224)
    float32 on the device, the DISTINCT mel-dB images of all windows, each spectrogram column computed once; first_rows /
    recording_index (host int64) and start_seconds (host float64) have one entry per window: images[first_rows[w] : first_rows[w]
    + 10] are the ten images of the window that starts start_seconds[w] into recordings[recording_index[w]].

    This is librosa's spectrogram of the whole TRACK (the recording up to the end of its last window), cut into images:
    power_to_db(melspectrogram(track, sr=22050, n_mels=224, hop_length=98)) with the track centre-padded by reflection at its own
    two ends and floored at the TRACK-wide maximum - 80 dB. Cropping 4 s pieces on the host and feeding them to
    recordings_to_clips + clips_to_images reflects at each crop's ends and floors against each crop's own maximum, so two things
    differ: the first image of a window in its columns 0..10 and the last in its columns 890..898 (the columns whose frames read
    reflected samples), and a window quieter than the track's loudest one sits on a higher floor. Everything else is the same
    samples through the same arithmetic, the same bits before the floor.

    Memory: the spectrogram is 896 B per column, about 0.2 MB per second of audio, and an image is 200 KB: for long recordings
    make the images in ranges (recordings_to_tracks + frontend.melspec_track_images), as Ensemble.score_image_timeline does.
    recordings / rates: as recordings_to_clips takes them, with its errors. Limits: a track of at most 2**30 samples, about 13.5
    hours, and at most 2**31 - 1 tiles of 256 samples in the batch; more raises ValueError. All errors come before anything is
    copied or launched. An empty sequence gives (0, 1, 224, 224) images."""
    return _track_images(*recordings_to_tracks(recordings, rates, hop_images))


def wavfiles_to_track_images(paths, hop_images=3):
    """16-bit WAV files -> recordings_to_track_images: read_wav16 on every path (other widths are refused)."""
    return _track_images(*wavfiles_to_tracks(paths, hop_images))


def audiofiles_to_track_images(paths, hop_images=3):
    """WAV files of any mixture of encodings read_audiofile accepts -> what recordings_to_track_images returns, the files' bytes
    decoded in the clips launch. Bit-identical to wavfiles_to_track_images for 16-bit files."""
    return _track_images(*audiofiles_to_tracks(paths, hop_images))


# ---- the VGGish branch on the librosa path: load_hdf5(cnn_type="vggish", use_librosa=True), dataset.py:232-243, :305-307, :316 -------
SAMPLES_NUM_VGGISH_LIBROSA = SR_VGGISH * 4       # 64 000: the reference's SAMPLES_NUM_VGGISH (params.py:10), the rows of this path
LIBROSA_N_MELS, LIBROSA_HOP, LIBROSA_FMIN, LIBROSA_FMAX, LIBROSA_TOP_DB = 64, 160, 125.0, 7500.0, 80.0


def create_spec_librosa(audio_array):
    """create_spec(audio_array, "vggish", 16000, ..., use_librosa=True, ...) of the reference (dataset.py:305-307, :316) for one
    clip of 16 kHz audio of any length from 2 048 samples on: librosa.feature.melspectrogram(y, sr=16000, n_mels=64,
    hop_length=160, center=False, htk=True, fmin=125, fmax=7500) + power_to_db -> (64, 1 + (n - 2048) // 160) float32 dB values on
    the device, clipped at the clip's maximum - 80. Shorter clips raise ValueError (librosa cannot frame them either)."""
    pcm = frontend.as_device_mono(audio_array)[None]
    return frontend.melspectrogram_db(pcm, SR_VGGISH, LIBROSA_N_MELS, LIBROSA_HOP, LIBROSA_TOP_DB, center=False, htk=True,
                                      fmin=LIBROSA_FMIN, fmax=LIBROSA_FMAX)[0]


def _librosa_overlap_only(what, overlap):
    if not overlap:
        raise ValueError("%s: overlap=False is not defined on the VGGish librosa path: the 388 columns give four whole 96-column "
                         "frames and a fifth of width 4, which the reference's split refuses (dataset.py:361)" % what)


def clips_to_frames_librosa(pcm, out_dtype=torch.float32):
    """(clips, 64 000) float32 device PCM at 16 kHz -> (clips, T, 1, 64, 96), the tensor load_hdf5(cnn_type="vggish",
    use_librosa=True) stores (dataset.py:243-254, mnemonic vggish_10_s) and Ensemble consumes, in TWO launches: the HTK mel-dB
    spectrogram of unpadded frames (388 columns) and the top_db clip + the ten overlapping windows 32 columns apart, written in
    `out_dtype` (float32 or bfloat16). Bit-identical to create_spec_librosa + split per clip. Rows are exactly 64 000 samples: the
    caller cuts longer clips and zero-fills shorter ones, as load_hdf5 means to."""
    assert pcm.dim() == 2
    if pcm.shape[1] != SAMPLES_NUM_VGGISH_LIBROSA:
        raise ValueError("clips_to_frames_librosa takes rows of exactly %d samples (%d s at %d Hz), got %d"
                         % (SAMPLES_NUM_VGGISH_LIBROSA, SAMPLES_NUM_VGGISH_LIBROSA // SR_VGGISH, SR_VGGISH, pcm.shape[1]))
    assert pcm.is_cuda
    if pcm.dtype != torch.float32:
        pcm = pcm.float()
    x_size = 96
    width = frontend.melspec_frames_librosa(SAMPLES_NUM_VGGISH_LIBROSA, LIBROSA_HOP)
    db, ws = frontend.melspec_db_unclipped_librosa(pcm, SR_VGGISH, LIBROSA_N_MELS, LIBROSA_HOP, LIBROSA_FMIN, LIBROSA_FMAX, True)
    return frontend.melspec_bags(db, ws, SAMPLES_NUM_VGGISH_LIBROSA, LIBROSA_HOP, LIBROSA_TOP_DB, T, x_size, (width - x_size) // (T - 1),
                                 out_dtype)


def recordings_to_frames_librosa(recordings, rates, overlap=True, out_dtype=torch.float32):
    """Recordings as they are decoded -> the (B, T, 1, 64, 96) bags of the VGGish librosa path in THREE launches whatever B is:
    recordings_to_clips at 16 kHz into rows of 64 000 samples (channel mean, resampy 'kaiser_best' resampling of the whole
    recording, cut at 4 s, zero fill), then clips_to_frames_librosa's two. recordings / rates: as recordings_to_clips takes them,
    with its errors. overlap=False raises ValueError. An empty sequence gives (0, T, 1, 64, 96)."""
    _librosa_overlap_only("recordings_to_frames_librosa", overlap)
    return _librosa_bags(recordings_to_clips(recordings, rates, SR_VGGISH, SAMPLES_NUM_VGGISH_LIBROSA), out_dtype)


def _librosa_bags(clips, out_dtype):
    if clips.shape[0] == 0:
        return torch.empty((0, T, 1, 64, 96), dtype=out_dtype, device=clips.device)
    return clips_to_frames_librosa(clips, out_dtype)


def wavfiles_to_frames_librosa(paths, overlap=True, out_dtype=torch.float32):
    """16-bit WAV files -> (B, T, 1, 64, 96) bags of the VGGish librosa path: read_wav16 on every path, then
    recordings_to_frames_librosa."""
    _librosa_overlap_only("wavfiles_to_frames_librosa", overlap)
    return recordings_to_frames_librosa(*_read_wav16s(paths), overlap, out_dtype)


def audiofiles_to_frames_librosa(paths, overlap=True, out_dtype=torch.float32):
    """WAV files of any mixture of encodings read_audiofile accepts -> (B, T, 1, 64, 96) bags of the VGGish librosa path, in three
    launches: audiofiles_to_clips at 16 kHz / 64 000 samples (the files' bytes decoded in the clips launch), then
    clips_to_frames_librosa's two."""
    _librosa_overlap_only("audiofiles_to_frames_librosa", overlap)
    return _librosa_bags(audiofiles_to_clips(paths, SR_VGGISH, SAMPLES_NUM_VGGISH_LIBROSA), out_dtype)
