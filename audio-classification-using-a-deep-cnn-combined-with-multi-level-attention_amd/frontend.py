"""Host side of the HIP audio front-end: device tables, buffer plumbing, ctypes calls.

PyTorch is used for device memory and streams only; all arithmetic is in csrc/logmel.hip.
"""

import collections
import ctypes

import numpy as np
import torch

from . import _lib

_tables = {}


def device_tables(device):
    """Constant tables of the fused kernel, built by the library in float64 and uploaded once."""
    key = str(device)
    if key not in _tables:
        L = _lib.lib()
        n = int(L.mla_logmel_table_floats())
        host = np.zeros(n, dtype=np.float32)
        _lib.check(L.mla_logmel_build_tables(host.ctypes.data_as(ctypes.c_void_p)))
        _tables[key] = torch.from_numpy(host).to(device)
    return _tables[key]


def counts(n_samples):
    """(stft_frames, examples) for a 16 kHz waveform; ValueError where the reference raises."""
    L = _lib.lib()
    f, e = ctypes.c_int64(), ctypes.c_int64()
    rc = L.mla_logmel_counts(int(n_samples), ctypes.byref(f), ctypes.byref(e))
    if rc == _lib.E_SHORT:
        raise ValueError("negative dimensions are not allowed")
    _lib.check(rc)
    return f.value, e.value


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("the HIP front-end needs a GPU (cuda:0); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def as_device_mono(data, pcm16=False):
    """ndarray / tensor, 1-D or (samples, channels) -> 1-D device tensor.

    pcm16=False (the public ``waveform_to_examples``, vggish_input.py:30-82, which never scales its input): integer
    arrays are converted to float32 VALUES as they are, like numpy's promotion in the reference.
    pcm16=True (``wavfile_to_examples`` and the PCM streaming paths, vggish_input.py:97-98 ``wav_data / 32768.0``): mono
    int16 stays int16 and the log-mel kernel scales by 1/32768 in its PCM read; multi-channel int16 is scaled in the mix.
    Multi-channel input is averaged over axis 1 as vggish_input.py:49-50 does, by `mla_mono_mix` on the device
    (double-precision mean, one rounding).
    """
    dev = _device()
    if isinstance(data, np.ndarray):
        if data.dtype != np.int16 or not pcm16:
            data = data.astype(np.float32, copy=False)     # float64 reference input: rounded once, like the mono path
        t = torch.from_numpy(np.array(data, order="C", copy=True) if not data.flags.writeable else np.ascontiguousarray(data)).to(dev)
    else:
        t = data.to(dev)
        if t.dtype != torch.int16 or not pcm16:
            t = t.float()
        t = t.contiguous()
    if t.dim() == 1:
        return t
    assert t.dim() == 2, "waveform must be 1-D or (samples, channels)"
    n, ch = t.shape
    out = torch.empty((n,), dtype=torch.float32, device=dev)
    code = _lib.I16 if t.dtype == torch.int16 else _lib.F32
    _lib.check(_lib.lib().mla_mono_mix(ctypes.c_void_p(t.data_ptr()), code, n, ch, ctypes.c_void_p(out.data_ptr()), _lib.stream_ptr()))
    return out


_resample_tables = {}


def kaiser_best_filter():
    """resampy's default interpolation filter 'kaiser_best' (resampy/filters.py sinc_window: 64 zero crossings, 2**9 table entries
    per crossing, Kaiser beta 14.769656459379492, rolloff 0.9475937167399596), right half, float64. resampy ships this table as a
    data file; it is host-side setup like the mel matrix. (interp_win, num_table)."""
    num_zeros, precision, beta, rolloff = 64, 9, 14.769656459379492, 0.9475937167399596
    num_bits = 2 ** precision
    n = num_bits * num_zeros
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    return np.kaiser(2 * n + 1, beta)[n:] * sinc_win, num_bits


_resample_filters = {}


def _resample_filter(ratio, gain=1.0):
    """The interpolation filter as the kernels read it, on the host in float64: 'kaiser_best' scaled by the ratio where it is < 1
    (resampy/core.py) and by `gain`, its first difference, entries per zero crossing. One per distinct (scale, gain): `resample`
    and `prepare_clips` upload the SAME values, which is what makes their outputs agree bit for bit."""
    key = (ratio if ratio < 1 else 1.0, float(gain))
    if key not in _resample_filters:
        win, num_table = kaiser_best_filter()
        if ratio < 1:
            win = win * ratio
        win = win * float(gain)
        delta = np.zeros_like(win)
        delta[:-1] = np.diff(win)
        _resample_filters[key] = (win, delta, num_table)
    return _resample_filters[key]


def resample(wave, sr_orig, sr_new, gain=1.0):
    """resampy.resample(wave, sr_orig, sr_new) (vggish_input.py:52-53) for a 1-D device waveform -> float32 device tensor of
    int(n * sr_new / sr_orig) samples, by the HIP kernel mla_resample (`gain` scales the filter table: the operation is linear).
    ValueError where resampy raises (bad rates, empty result)."""
    if sr_orig <= 0:
        raise ValueError("Invalid sample rate: sr_orig=%r" % (sr_orig,))
    if sr_new <= 0:
        raise ValueError("Invalid sample rate: sr_new=%r" % (sr_new,))
    assert wave.dim() == 1 and wave.is_cuda
    wave = wave.float().contiguous()
    ratio = float(sr_new) / float(sr_orig)
    L = _lib.lib()
    n_out = int(L.mla_resample_length(wave.shape[0], float(sr_orig), float(sr_new)))
    if n_out < 1:
        raise ValueError("Input signal length=%d is too small to resample from %s->%s" % (wave.shape[0], sr_orig, sr_new))
    key = (str(wave.device), ratio if ratio < 1 else 1.0, float(gain))
    if key not in _resample_tables:
        win, delta, num_table = _resample_filter(ratio, gain)
        _resample_tables[key] = (torch.from_numpy(win).to(wave.device), torch.from_numpy(delta).to(wave.device), num_table)
    win, delta, num_table = _resample_tables[key]
    out = torch.empty(n_out, dtype=torch.float32, device=wave.device)
    vp = ctypes.c_void_p
    _lib.check(L.mla_resample(vp(wave.data_ptr()), wave.shape[0], float(sr_orig), float(sr_new), vp(win.data_ptr()), vp(delta.data_ptr()),
                              win.shape[0], num_table, vp(out.data_ptr()), n_out, _lib.stream_ptr()))
    return out


_clips_tables = {}


def _host_array(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()           # a device tensor is read back (one synchronisation); host arrays cost nothing
    return np.ascontiguousarray(np.asarray(a), dtype=dtype).reshape(-1)


def clips_table_index(rates, sr_out):
    """(the distinct filter scales of a batch in order of first use, each recording's index into them). A recording at sr_out
    is not filtered and keeps index 0; a rate <= 0 is left for the library to refuse."""
    scales, tab = [], np.zeros(len(rates), dtype=np.int32)
    for i, r in enumerate(rates):
        if r > 0 and r != sr_out:
            ratio = float(sr_out) / float(r)
            key = ratio if ratio < 1 else 1.0
            if key not in scales:
                scales.append(key)
            tab[i] = scales.index(key)
    return tuple(scales), tab


def clips_tables_host(scales):
    """The filter tables of `scales` back to back as mla_clips_prepare reads them: per table nwin (win, delta) pairs, float64."""
    if not scales:
        return np.zeros(0, dtype=np.float64)
    return np.concatenate([np.stack(_resample_filter(k)[:2], axis=1).reshape(-1) for k in scales])


def _clips_launch(label, packed, off, fr, ch, rt, fm, sr_out, samples_num, out):
    """The launch behind prepare_clips (fm None: mla_clips_prepare, `off` in elements) and prepare_clips_raw (fm the format codes:
    mla_clips_prepare_raw, `off` in bytes). The filter tables of the batch's scales are cached on the device; the descriptors
    travel in one pinned buffer, offsets | frames | rates | channels | table index [| formats], and one copy."""
    dev = packed.device
    B = fr.shape[0]
    assert all(a.shape[0] == B for a in (off, ch, rt) + (() if fm is None else (fm,))), "one descriptor entry per recording"
    sr_out, samples_num = float(sr_out), int(samples_num)
    if out is None:
        out = torch.empty((B, samples_num), dtype=torch.float32, device=dev)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (B, samples_num)
    if B == 0:
        return out
    scales, tab = clips_table_index(rt, sr_out)
    nwin, num_table = _resample_filter(1.0)[0].shape[0], _resample_filter(1.0)[2]
    tkey = (str(dev), scales)
    if tkey not in _clips_tables:
        _clips_tables[tkey] = torch.from_numpy(clips_tables_host(scales)).to(dev)
    cols = [off, fr, ch, rt, tab] + ([] if fm is None else [fm])            # in the order the C entries take them
    desc = torch.empty(sum(a.nbytes for a in cols), dtype=torch.uint8, pin_memory=True)
    h, at, pos = desc.numpy(), [0] * len(cols), 0
    for i in sorted(range(len(cols)), key=lambda i: -cols[i].itemsize):       # the 8-byte columns first, so every one is aligned
        at[i] = pos
        h[pos:pos + cols[i].nbytes].view(cols[i].dtype)[:] = cols[i]
        pos += cols[i].nbytes
    d = desc.to(dev, non_blocking=True)
    vp = ctypes.c_void_p
    L = _lib.lib()
    if fm is None:
        entry = (L.mla_clips_prepare, vp(packed.data_ptr()), _lib.I16 if packed.dtype == torch.int16 else _lib.F32, packed.shape[0])
    else:
        entry = (L.mla_clips_prepare_raw, vp(packed.data_ptr()), packed.shape[0])
    from . import ops
    _lib.check(ops._timed(label, *entry, B, *[vp(d.data_ptr() + o) for o in at], *[a.ctypes.data_as(vp) for a in cols], sr_out, samples_num,
                          vp(_clips_tables[tkey].data_ptr()) if scales else None, len(scales), nwin, num_table, vp(out.data_ptr()),
                          _lib.stream_ptr()))
    return out


def prepare_clips(packed, offsets, frames, channels, rates, sr_out, samples_num, out=None):
    """A batch of ragged recordings -> (B, samples_num) float32 clips at `sr_out` in ONE launch of csrc/clips.hip: channel mean,
    resampy 'kaiser_best' resampling of the whole recording (a copy where the rate already is sr_out), cut at samples_num and
    zero fill -- librosa.load(path, sr=sr_out) followed by dataset.py:233-237 of the reference.

    packed: 1-D device tensor, int16 (scaled by 1/32768) or float32, the recordings' interleaved frames back to back.
    offsets / frames / channels / rates: per recording, the element index of its first sample in `packed`, its frames, its
    channel count and its rate in Hz. They are needed on BOTH sides (the library validates and sizes LDS on the host, the
    kernel reads them on the device): pass host arrays where you have them (dataset.recordings_to_clips does); device tensors
    are read back first. They travel to the device in one pinned buffer and one copy. Every row depends on its own recording
    only and equals `resample(as_device_mono(x), rate, sr_out)` cut and zero-filled, bit for bit. `out`, when given, is
    overwritten completely."""
    assert packed.is_cuda and packed.dim() == 1 and packed.is_contiguous() and packed.dtype in (torch.int16, torch.float32)
    return _clips_launch("clips_prepare", packed, _host_array(offsets, np.int64), _host_array(frames, np.int64),
                         _host_array(channels, np.int32), _host_array(rates, np.float64), None, sr_out, samples_num, out)


def prepare_clips_raw(packed_bytes, byte_offsets, frames, channels, rates, formats, sr_out, samples_num, out=None):
    """prepare_clips for recordings that still are the bytes of their files' data chunks: the samples are decoded in the same
    ONE launch (csrc/clips.hip, the same clips_kernel), so a batch of mixed encodings is uploaded as it sits on disk.

    packed_bytes: 1-D uint8 device tensor, the data chunks (little endian, interleaved frames). byte_offsets: where each
    recording starts, a multiple of its sample size. formats: one code per recording, _lib.U8 / I16 / I24 / I32 (PCM, scaled
    to [-1, 1)) or _lib.F32 / F64 (float64 samples are rounded to float32 one by one). The other arguments, the descriptor
    traffic and the cached filter tables are prepare_clips's. A row equals prepare_clips's on the recording decoded to float32
    first, bit for bit, for every format but multi-channel 32-bit PCM, whose integers are summed exactly and rounded once. No byte
    outside a recording's own range is read. `out`, when given, is overwritten completely."""
    assert packed_bytes.is_cuda and packed_bytes.dim() == 1 and packed_bytes.is_contiguous() and packed_bytes.dtype == torch.uint8
    return _clips_launch("clips_prepare_raw", packed_bytes, _host_array(byte_offsets, np.int64), _host_array(frames, np.int64),
                         _host_array(channels, np.int32), _host_array(rates, np.float64), _host_array(formats, np.int32),
                         sr_out, samples_num, out)


def waveforms_to_examples(pcm, out_dtype=torch.float32, out=None):
    """(W, n) device PCM (float32 or int16) -> (W * N, 96, 64) examples, waveform-major."""
    assert pcm.dim() == 2 and pcm.is_cuda and pcm.stride(1) == 1
    n_wave, n_samples = pcm.shape
    _, n_ex = counts(n_samples)
    if out is None:
        out = torch.empty((n_wave * n_ex, 96, 64), dtype=out_dtype, device=pcm.device)
    else:
        assert out.is_contiguous() and out.numel() == n_wave * n_ex * 96 * 64 and out.dtype == out_dtype
    if n_wave * n_ex == 0:
        return out
    pcm_code = {torch.float32: _lib.F32, torch.int16: _lib.I16}[pcm.dtype]
    out_code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}[out_dtype]
    tab = device_tables(pcm.device)
    from . import ops
    _lib.check(ops._timed("logmel", _lib.lib().mla_logmel_examples,
                          ctypes.c_void_p(pcm.data_ptr()), pcm_code, n_wave, n_samples, pcm.stride(0) if n_wave > 1 else n_samples,   # (a size-1 dimension's stride is arbitrary)
                          ctypes.c_void_p(tab.data_ptr()), ctypes.c_void_p(out.data_ptr()), out_code, _lib.stream_ptr()))
    return out


_bwd_tables = {}


def device_bwd_tables(device):
    """Constant tables of the log-mel backward kernel (transposed mel step, split twiddles), built by the library in float64."""
    key = str(device)
    if key not in _bwd_tables:
        L = _lib.lib()
        host = np.zeros(int(L.mla_logmel_bwd_table_floats()), dtype=np.float32)
        _lib.check(L.mla_logmel_bwd_build_tables(host.ctypes.data_as(ctypes.c_void_p)))
        _bwd_tables[key] = torch.from_numpy(host).to(device)
    return _bwd_tables[key]


def waveforms_to_examples_backward(pcm, grad_examples, out=None):
    """The gradient of ``waveforms_to_examples(pcm)`` (float32 examples) with respect to the waveform: (W, n) device PCM (float32, or
    int16 meaning pcm / 32768: the gradient is with respect to that float value) and grad_examples (W * N, 96, 64) float32 ->
    (W, n) float32, one launch of csrc/logmel_bwd.hip. The frames' spectra are recomputed from `pcm`. Every element of the result
    is stored exactly once -- samples behind the last used frame get 0.0 -- so `out`, when given ((W, n) float32, unit stride
    along the samples), needs no zeroing; the result is deterministic and a row's bits do not depend on the batch.

    Conditioning: the function passes a bin's gradient along its unit phasor X_k / |X_k|, which float32 only knows where |X_k| is
    well above the frame's rounding noise. On noise-like audio the result is within ~1e-6 of the float64 gradient; on a pure tone,
    whose bins lie at 1e-17 of the peak, any float32 evaluation (torch's included) is tens of percent off. NaN / Inf in either
    input are outside the contract."""
    assert pcm.dim() == 2 and pcm.is_cuda and pcm.stride(1) == 1 and pcm.dtype in (torch.float32, torch.int16)
    n_wave, n_samples = pcm.shape
    _, n_ex = counts(n_samples)
    g = grad_examples
    assert g.is_cuda and g.dtype == torch.float32 and g.numel() == n_wave * n_ex * 96 * 64, "grad_examples must be (W * N, 96, 64) float32"
    g = g.contiguous()
    if out is None:
        out = torch.empty((n_wave, n_samples), dtype=torch.float32, device=pcm.device)
    else:
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n_wave, n_samples) and (n_samples == 0 or out.stride(1) == 1)
    if n_wave == 0:
        return out
    pcm_code = {torch.float32: _lib.F32, torch.int16: _lib.I16}[pcm.dtype]
    vp = ctypes.c_void_p
    from . import ops
    _lib.check(ops._timed("logmel_bwd", _lib.lib().mla_logmel_examples_bwd,
                          vp(pcm.data_ptr()), pcm_code, n_wave, n_samples, pcm.stride(0) if n_wave > 1 else n_samples,
                          vp(device_tables(pcm.device).data_ptr()), vp(device_bwd_tables(pcm.device).data_ptr()),
                          vp(g.data_ptr()) if g.numel() else None, vp(out.data_ptr()), out.stride(0) if n_wave > 1 else n_samples,
                          _lib.stream_ptr()))
    return out


def waveforms_to_examples_differentiable(pcm):
    """``waveforms_to_examples`` behind autograd: (W, n) float32 device PCM that may require grad -> (W * N, 96, 64) float32
    examples attached to the graph (differentiable.LogMelFn: the forward is the same launch and gives the same bits, the backward
    is waveforms_to_examples_backward). With ``set_input_grad(True)`` on the model the reference's literal loop fills pcm.grad:

        ex = waveforms_to_examples_differentiable(pcm); loss = crit(clf(ex.view(B, T, 1, 96, 64)), y); loss.backward()
    """
    from . import differentiable
    return differentiable.LogMelFn.apply(pcm)


def logmel_bags(pcm, counts, n_frames=10, stride=32, out_dtype=torch.float32, out=None):
    """(B, n) device rows of 16 kHz mono PCM (float32 or int16) holding counts[c] <= 4 whole 0.96 s examples each -> the
    (B, n_frames, 1, 64, 96) bag tensor of the reference's native VGGish dataset path (dataset.py:318-324 create_spec + :329-363
    split) in ONE launch of csrc/logmel.hip (logmel_bags_kernel): log-mel of the examples a row has, 0.0 in the slots it lacks, cut
    into n_frames windows of 96 columns at `stride` -- (10, 32) with overlap, (4, 96) without. Written directly in `out_dtype`
    (float32 or bfloat16). counts: host integers (a device tensor is read back first); they travel in one pinned buffer and one
    copy. Row c equals mla_logmel_examples + mla_dataset_frames on its first 15 600 + 15 360 (counts[c] - 1) samples, bit for bit;
    nothing beyond them is read. `out`, when given, is overwritten completely."""
    assert pcm.dim() == 2 and pcm.is_cuda and (pcm.shape[1] <= 1 or pcm.stride(1) == 1) and pcm.dtype in (torch.float32, torch.int16)
    B, n = pcm.shape
    cnt = _host_array(counts, np.int32)
    assert cnt.shape[0] == B, "one count per row"
    n_frames, stride = int(n_frames), int(stride)
    if out is None:
        out = torch.empty((B, n_frames, 1, 64, 96), dtype=out_dtype, device=pcm.device)
    else:
        assert out.is_cuda and out.is_contiguous() and out.dtype == out_dtype and tuple(out.shape) == (B, n_frames, 1, 64, 96)
    if B == 0:
        return out
    pcm_code = {torch.float32: _lib.F32, torch.int16: _lib.I16}[pcm.dtype]
    out_code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}[out_dtype]
    tab = device_tables(pcm.device)
    host = torch.empty(B, dtype=torch.int32, pin_memory=True)
    host.numpy()[:] = cnt
    d = host.to(pcm.device, non_blocking=True)
    vp = ctypes.c_void_p
    from . import ops
    _lib.check(ops._timed("logmel_bags", _lib.lib().mla_logmel_bags, vp(pcm.data_ptr()), pcm_code, B, n, pcm.stride(0) if B > 1 else n,
                          vp(d.data_ptr()), cnt.ctypes.data_as(vp), n_frames, stride, vp(tab.data_ptr()), vp(out.data_ptr()), out_code,
                          _lib.stream_ptr()))
    return out


def timeline_counts(n_samples, hop_slots):
    """(windows, kept slots, samples read) of a 16 kHz recording of n_samples scored at a hop of hop_slots * 0.32 s
    (mla_timeline_counts, the single source of the arithmetic; include/mla_hip.h states it). ValueError for fewer than 240
    samples, where the reference raises, and for hop_slots < 1."""
    if int(hop_slots) != hop_slots or hop_slots < 1:
        raise ValueError("hop_slots must be an integer >= 1 (the hop is hop_slots * 0.32 s), got %r" % (hop_slots,))
    w, s, r = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    rc = _lib.lib().mla_timeline_counts(int(n_samples), int(hop_slots), ctypes.byref(w), ctypes.byref(s), ctypes.byref(r))
    if rc == _lib.E_SHORT:
        raise ValueError("negative dimensions are not allowed")
    _lib.check(rc)
    return w.value, s.value, r.value


def timeline_descriptors(n_valid, hop_slots):
    """The (R, 5) int64 descriptors mla_logmel_timeline takes for recordings of n_valid[i] samples at 16 kHz -- first_slot, cols,
    spec_cols, first_item, q per recording -- with (the windows of each, all kept slots, the most samples a row must hold)."""
    q = int(hop_slots)
    desc = np.zeros((len(n_valid), 5), dtype=np.int64)
    windows = np.zeros(len(n_valid), dtype=np.int64)
    slot, item, most = 0, 0, 0
    for i, n in enumerate(n_valid):
        w, s, read = timeline_counts(int(n), q)
        cols = 32 * q * (w - 1) + 384
        desc[i] = (slot, cols, max(read - 240, 0) // 160, item, q)      # `read` samples = 160 spec_cols + 240, or none
        windows[i] = w
        slot += s
        item += 48 + min(4 * q, 48) * (w - 1)
        most = max(most, read)
    return desc, windows, slot, most


def logmel_timeline(pcm, n_valid, hop_slots=3, out_dtype=torch.float32, out=None):
    """(R, n) device rows of 16 kHz mono PCM (float32 or int16), row i a recording of n_valid[i] samples of which the row holds at
    least timeline_counts(n_valid[i], hop_slots)[2] -> (slots, first_rows, recording_index) in ONE launch of csrc/logmel.hip
    (logmel_timeline_kernel). slots: (S, 64, 96) in `out_dtype` (float32 or bfloat16), the DISTINCT 96-column slots of every
    recording's windows at a hop of hop_slots * 0.32 s, each log-mel column computed once. first_rows / recording_index: host
    int64 arrays with one entry per window, recordings in order and windows in order of time: slots[first_rows[w] : first_rows[w]
    + 10] is window w's bag, bit for bit what logmel_bags gives for the crop pcm[i, 5120 * hop_slots * j :][: 61680] (a recording
    of fewer than 61 680 samples has one window, its logmel_bags bag). n_valid: host integers (a device tensor is read back
    first); the descriptors travel in one pinned buffer and one copy. Nothing beyond the samples counted is read. `out`, when
    given, is overwritten completely."""
    assert pcm.dim() == 2 and pcm.is_cuda and (pcm.shape[1] <= 1 or pcm.stride(1) == 1) and pcm.dtype in (torch.float32, torch.int16)
    R, n = pcm.shape
    nv = _host_array(n_valid, np.int64)
    assert nv.shape[0] == R, "one length per row"
    desc, windows, total, _ = timeline_descriptors(nv, hop_slots)
    if out is None:
        out = torch.empty((total, 64, 96), dtype=out_dtype, device=pcm.device)
    else:
        assert out.is_cuda and out.is_contiguous() and out.dtype == out_dtype and tuple(out.shape) == (total, 64, 96)
    recording_index = np.repeat(np.arange(R, dtype=np.int64), windows)
    step = min(int(hop_slots), 10)
    first_rows = np.concatenate([desc[i, 0] + step * np.arange(windows[i], dtype=np.int64) for i in range(R)]) if R else np.zeros(0, np.int64)
    if R == 0:
        return out, first_rows, recording_index
    pcm_code = {torch.float32: _lib.F32, torch.int16: _lib.I16}[pcm.dtype]
    out_code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}[out_dtype]
    tab = device_tables(pcm.device)
    host = torch.empty(desc.size, dtype=torch.int64, pin_memory=True)
    host.numpy()[:] = desc.reshape(-1)
    d = host.to(pcm.device, non_blocking=True)
    vp = ctypes.c_void_p
    from . import ops
    _lib.check(ops._timed("logmel_timeline", _lib.lib().mla_logmel_timeline, vp(pcm.data_ptr()), pcm_code, R, n, pcm.stride(0) if R > 1 else n,
                          vp(d.data_ptr()), desc.ctypes.data_as(vp), total, vp(tab.data_ptr()), vp(out.data_ptr()), out_code,
                          _lib.stream_ptr()))
    return out, first_rows, recording_index


_melspec_tables = {}
MELSPEC_AMIN = 1e-10     # librosa.power_to_db's default amin (ref = 1.0)


def melspec_tables(device, sr, n_mels):
    """Window, twiddles and the sparse Slaney mel basis for (sr, n_mels), built by the library in float64 and uploaded once."""
    key = (str(device), float(sr), int(n_mels))
    if key not in _melspec_tables:
        L = _lib.lib()
        n = int(L.mla_melspec_table_floats(float(sr), int(n_mels)))
        if n < 0:
            raise ValueError("melspectrogram_db needs sr > 0 and 1 <= n_mels <= 1024 (got sr=%r, n_mels=%r)" % (sr, n_mels))
        host = np.zeros(n, dtype=np.float32)
        _lib.check(L.mla_melspec_build_tables(float(sr), int(n_mels), host.ctypes.data_as(ctypes.c_void_p)))
        _melspec_tables[key] = torch.from_numpy(host).to(device)
    return _melspec_tables[key]


def melspec_frames(n_samples, hop_length):
    return int(_lib.lib().mla_melspec_frames(int(n_samples), int(hop_length)))


def melspec_db_unclipped(pcm, sr, n_mels, hop_length):
    """(clips, n) device PCM -> ((clips, n_mels, frames) dB values before the top_db clip, the workspace of per-clip partial
    maxima that melspec_images reads). Kernel 1 of the ResNet branch's front-end (csrc/melspec.hip)."""
    assert pcm.dim() == 2 and pcm.is_cuda and pcm.dtype == torch.float32 and (pcm.shape[1] <= 1 or pcm.stride(1) == 1)
    clips, n = pcm.shape
    L = _lib.lib()
    tab = melspec_tables(pcm.device, sr, n_mels)
    ws_bytes = int(L.mla_melspec_workspace_bytes(clips, n, int(hop_length)))
    frames = melspec_frames(n, hop_length)
    if ws_bytes < 0 or frames < 0:
        raise ValueError("hop_length must be a positive integer (got %r)" % (hop_length,))
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=pcm.device)
    db = torch.empty((clips, int(n_mels), frames), dtype=torch.float32, device=pcm.device)
    vp = ctypes.c_void_p
    from . import ops
    _lib.check(ops._timed("melspec_db", L.mla_melspec_db, vp(pcm.data_ptr()), clips, n, pcm.stride(0) if clips > 1 else n, int(hop_length),
                          int(n_mels), MELSPEC_AMIN, vp(tab.data_ptr()), vp(db.data_ptr()), vp(ws.data_ptr()), _lib.stream_ptr()))
    return db, ws


def melspec_images(db, ws, n_samples, hop_length, top_db, n_images, image_w, image_stride):
    """power_to_db's clip against the clip-wide maximum + split: (clips, n_mels, frames) -> (clips, n_images, 1, n_mels, image_w).
    Kernel 2 of the ResNet branch's front-end: a select and a gather, bit-determined by `db`."""
    clips, n_mels, _ = db.shape
    out = torch.empty((clips, int(n_images), 1, n_mels, int(image_w)), dtype=torch.float32, device=db.device)
    vp = ctypes.c_void_p
    from . import ops
    _lib.check(ops._timed("melspec_images", _lib.lib().mla_melspec_images, vp(db.data_ptr()), vp(ws.data_ptr()), clips, int(n_samples),
                          int(hop_length), n_mels, float(top_db), int(n_images), int(image_w), int(image_stride), vp(out.data_ptr()),
                          _lib.stream_ptr()))
    return out


def melspec_images_backward(grad_images, db, ws, n_samples, hop_length, top_db, n_images, image_w, image_stride, floor_grad=True, out=None):
    """The gradient of ``melspec_images`` with respect to `db`: grad_images (clips, n_images, 1, n_mels, image_w) float32, with the
    `db` and `ws` of melspec_db_unclipped -> d_db (clips, n_mels, frames). Overlapping images add; a cell below the floor passes
    nothing. floor_grad=True (torch.autograd's answer) adds the floor's own gradient, the sum over the clipped cells, to the cell
    that holds the clip's maximum (the first in (band, column) order where several do); floor_grad=False treats the floor as a
    constant. One launch of csrc/melspec_bwd.hip; every element is stored exactly once, so `out`, when given (contiguous, db's shape),
    needs no zeroing."""
    clips, n_mels, frames = db.shape
    g = grad_images
    assert g.is_cuda and g.dtype == torch.float32 and g.numel() == clips * int(n_images) * n_mels * int(image_w), \
        "grad_images must be (clips, n_images, 1, n_mels, image_w) float32"
    g = g.contiguous()
    if out is None:
        out = torch.empty((clips, n_mels, frames), dtype=torch.float32, device=db.device)
    else:
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == tuple(db.shape) and out.is_contiguous()
    d_db = out
    vp = ctypes.c_void_p
    from . import ops
    _lib.check(ops._timed("melspec_images_bwd", _lib.lib().mla_melspec_images_bwd, vp(g.data_ptr()), vp(db.data_ptr()), vp(ws.data_ptr()), clips,
                          int(n_samples), int(hop_length), n_mels, float(top_db), int(n_images), int(image_w), int(image_stride),
                          int(bool(floor_grad)), vp(d_db.data_ptr()), _lib.stream_ptr()))
    return d_db


def melspec_db_backward(pcm, d_db, sr, n_mels, hop_length, out=None):
    """The gradient of ``melspec_db_unclipped`` with respect to the waveform: (clips, n) float32 device PCM and d_db (clips, n_mels,
    frames) -> d_pcm (clips, n) float32. The frames' spectra are recomputed from `pcm`; a band whose power is at or below amin
    passes nothing (an all-zero clip gives exact zeros). Every sample is stored exactly once, so `out`, when given ((clips, n)
    float32, unit stride along the samples), needs no zeroing; deterministic, and a row's bits do not depend on the batch."""
    assert pcm.dim() == 2 and pcm.is_cuda and pcm.dtype == torch.float32 and (pcm.shape[1] <= 1 or pcm.stride(1) == 1)
    clips, n = pcm.shape
    L = _lib.lib()
    ws_bytes = int(L.mla_melspec_bwd_workspace_bytes(clips, n, int(hop_length), int(n_mels)))
    frames = melspec_frames(n, hop_length)
    if ws_bytes < 0 or frames < 0:
        raise ValueError("hop_length must be a positive integer (got %r)" % (hop_length,))
    assert d_db.is_cuda and d_db.dtype == torch.float32 and tuple(d_db.shape) == (clips, int(n_mels), frames), "d_db must be (clips, n_mels, frames) float32"
    d_db = d_db.contiguous()
    if out is None:
        out = torch.empty((clips, n), dtype=torch.float32, device=pcm.device)
    else:
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (clips, n) and (n <= 1 or out.stride(1) == 1)
    tab = melspec_tables(pcm.device, sr, n_mels)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=pcm.device)
    vp = ctypes.c_void_p
    from . import ops
    _lib.check(ops._timed("melspec_db_bwd", L.mla_melspec_db_bwd, vp(pcm.data_ptr()), clips, n, pcm.stride(0) if clips > 1 else n, int(hop_length),
                          int(n_mels), MELSPEC_AMIN, vp(tab.data_ptr()), vp(d_db.data_ptr()), vp(ws.data_ptr()), vp(out.data_ptr()),
                          out.stride(0) if clips > 1 else n, _lib.stream_ptr()))
    return out


def melspectrogram_db_backward(pcm, grad_db, sr, n_mels, hop_length, top_db=80.0, floor_grad=True, center=True, htk=False, fmin=0.0, fmax=None):
    """The gradient of ``melspectrogram_db(pcm, sr, n_mels, hop_length, top_db)`` with respect to `pcm`: grad_db (clips, n_mels,
    frames) float32 -> (clips, n) float32; top_db=None differentiates the unclipped spectrogram. The forward's two kernels run again
    (the spectrogram and its maxima are not kept), then the two backward launches. Built for the centred spectrogram with librosa's
    default Slaney basis only: the HTK / center=False path of the VGGish librosa branch is out of scope."""
    if not center or htk or fmin != 0.0 or (fmax is not None and float(fmax) != float(sr) / 2):
        raise NotImplementedError("melspectrogram_db_backward differentiates the centred spectrogram with librosa's default mel basis "
                                  "(center=True, htk=False, fmin=0, fmax=sr/2); the HTK / center=False path of the VGGish librosa branch "
                                  "is out of scope")
    if pcm.shape[1] < 1025:
        raise ValueError("melspectrogram_db_backward needs at least 1025 samples per clip (got %d)" % pcm.shape[1])
    if top_db is not None and top_db < 0:
        raise ValueError("top_db must be non-negative")
    if top_db is None:
        return melspec_db_backward(pcm, grad_db, sr, n_mels, hop_length)
    db, ws = melspec_db_unclipped(pcm, sr, n_mels, hop_length)
    d_db = melspec_images_backward(grad_db, db, ws, pcm.shape[1], hop_length, top_db, 1, db.shape[2], 0, floor_grad)
    return melspec_db_backward(pcm, d_db, sr, n_mels, hop_length)


# ---- the ResNet branch over time: tracks of recordings of any length and the distinct images of their windows ----
TRACK_SR, TRACK_MELS, TRACK_HOP, TRACK_IMAGE_W, TRACK_IMAGE_STEP, TRACK_WINDOW_IMAGES = 22050, 224, 98, 224, 75, 10

TrackDescriptors = collections.namedtuple("TrackDescriptors", "host device windows images columns runs most")
Track = collections.namedtuple("Track", "db maxima descriptors first_rows recording_index")


def melspec_track_counts(n, hop_images):
    """(windows, kept images, track samples L, track columns C) of a recording of n samples at 22 050 Hz scored in 4 s windows
    hop_images / 3 s apart (mla_melspec_track_counts, the single source of the arithmetic; include/mla_hip.h states it).
    n >= 88 200: windows = 1 + (n - 88 200) // (7 350 * hop_images); n < 88 200: one window, the recording zero-filled.
    L = 88 200 + 7 350 * hop_images * (windows - 1), C = 1 + L // 98. ValueError for n < 0 and for a hop_images that is no integer
    >= 1."""
    if int(hop_images) != hop_images or hop_images < 1:
        raise ValueError("hop_images must be an integer >= 1 (the hop is hop_images / 3 s), got %r" % (hop_images,))
    if n < 0:
        raise ValueError("a recording cannot have %r samples" % (n,))
    w, s, l, c = (ctypes.c_int64() for _ in range(4))
    _lib.check(_lib.lib().mla_melspec_track_counts(int(n), int(hop_images), ctypes.byref(w), ctypes.byref(s), ctypes.byref(l), ctypes.byref(c)))
    return w.value, s.value, l.value, c.value


def melspec_track_descriptors(lengths, hop_images):
    """The descriptors mla_melspec_track_db and mla_melspec_track_images take for recordings of lengths[i] samples at 22 050 Hz:
    TrackDescriptors(host, device, windows, images, columns, runs, most) with host the (R, 6) int64 array -- track samples,
    columns, first_run, db_offset, first_image, hop_images per recording --, device None (melspec_track_db uploads it), windows
    the (R,) window counts, and the batch's kept images, columns, runs of 16 columns and longest track."""
    q = int(hop_images)
    desc = np.zeros((len(lengths), 6), dtype=np.int64)
    windows = np.zeros(len(lengths), dtype=np.int64)
    run, col, image, most = 0, 0, 0, 0
    for i, n in enumerate(lengths):
        w, s, l, c = melspec_track_counts(int(n), hop_images)
        desc[i] = (l, c, run, TRACK_MELS * col, image, q)
        windows[i] = w
        run += (c + 15) // 16
        col += c
        image += s
        most = max(most, l)
    return TrackDescriptors(desc, None, windows, image, col, run, most)


def melspec_track_db(pcm, lengths, hop_images):
    """(R, n) float32 device rows at 22 050 Hz, row i a recording of lengths[i] samples zero-filled to at least 88 200 (what
    dataset.recordings_to_clips(..., samples_num=the longest track) gives) -> Track(db, maxima, descriptors, first_rows,
    recording_index) in TWO launches of csrc/melspec.hip whatever the batch is (melspec_track_db_kernel over the runs of all
    tracks, melspec_track_max_kernel with one workgroup per recording).

    db: flat float32, recording i's unclipped dB spectrogram of its track -- its first L_i samples, reflected at ITS ends -- as a
    band-major (224, C_i) block at descriptors.host[i, 3]; maxima: (R,) its maximum, NaN where the track has one. first_rows /
    recording_index: host int64, one entry per window, recordings in order and windows in order of time: the images of window w
    are rows first_rows[w] .. first_rows[w] + 9 of melspec_track_images. lengths: host integers (a device tensor is read back
    first); the descriptors travel in one pinned buffer and one copy. Memory: 896 B per column, about 0.2 MB per second of audio.
    Nothing at or behind L_i of a row is read, and a recording's values are the same bits alone, in any batch and at any position."""
    assert pcm.dim() == 2 and pcm.is_cuda and pcm.dtype == torch.float32 and (pcm.shape[1] <= 1 or pcm.stride(1) == 1)
    R, n = pcm.shape
    nv = _host_array(lengths, np.int64)
    assert nv.shape[0] == R, "one length per row"
    d = melspec_track_descriptors(nv, hop_images)
    step = min(int(hop_images), TRACK_WINDOW_IMAGES)
    recording_index = np.repeat(np.arange(R, dtype=np.int64), d.windows)
    first_rows = np.concatenate([d.host[i, 4] + step * np.arange(d.windows[i], dtype=np.int64) for i in range(R)]) if R else np.zeros(0, np.int64)
    db = torch.empty(TRACK_MELS * d.columns, dtype=torch.float32, device=pcm.device)
    maxima = torch.empty(R, dtype=torch.float32, device=pcm.device)
    if R == 0:
        return Track(db, maxima, d, first_rows, recording_index)
    ws = torch.empty(d.runs, dtype=torch.float32, device=pcm.device)
    tab = melspec_tables(pcm.device, TRACK_SR, TRACK_MELS)
    host = torch.empty(d.host.size, dtype=torch.int64, pin_memory=True)
    host.numpy()[:] = d.host.reshape(-1)
    d = d._replace(device=host.to(pcm.device, non_blocking=True))
    vp = ctypes.c_void_p
    from . import ops
    _lib.check(ops._timed("melspec_track_db", _lib.lib().mla_melspec_track_db, vp(pcm.data_ptr()), R, n, pcm.stride(0) if R > 1 else n,
                          vp(d.device.data_ptr()), d.host.ctypes.data_as(vp), d.columns, MELSPEC_AMIN, vp(tab.data_ptr()), vp(db.data_ptr()),
                          vp(ws.data_ptr()), vp(maxima.data_ptr()), _lib.stream_ptr()))
    return Track(db, maxima, d, first_rows, recording_index)


def melspec_track_images(track, first, count, top_db=80.0):
    """The kept images with global row in [first, first + count) of a Track -> (count, 1, 224, 224) float32 in ONE launch
    (melspec_track_images_kernel): a select against the TRACK-wide maximum and a gather, out[i][0][b][x] = max(D_r[b][75 u + x],
    max(D_r) - top_db), bit-determined by track.db. The range lets the caller make the images chunk by chunk: an image is 200 KB."""
    d = track.descriptors
    first, count = int(first), int(count)
    if first < 0 or count < 0 or first + count > d.images:
        raise ValueError("images %d .. %d leave the %d kept images of the track" % (first, first + count, d.images))
    out = torch.empty((count, 1, TRACK_MELS, TRACK_IMAGE_W), dtype=torch.float32, device=track.db.device)
    if count == 0:
        return out
    vp = ctypes.c_void_p
    from . import ops
    _lib.check(ops._timed("melspec_track_images", _lib.lib().mla_melspec_track_images, vp(track.db.data_ptr()), vp(track.maxima.data_ptr()),
                          d.host.shape[0], vp(d.device.data_ptr()), d.host.ctypes.data_as(vp), d.columns, float(top_db), first, count,
                          vp(out.data_ptr()), _lib.stream_ptr()))
    return out


def melspec_band_tables(device, sr, n_mels, fmin, fmax, htk):
    """melspec_tables for any mel basis librosa.filters.mel(sr, 2048, n_mels, fmin, fmax, htk) builds (norm="slaney")."""
    key = (str(device), float(sr), int(n_mels), float(fmin), float(fmax), bool(htk))
    if key not in _melspec_tables:
        L = _lib.lib()
        cfg = (float(sr), int(n_mels), float(fmin), float(fmax), int(bool(htk)))
        n = int(L.mla_melspec_band_table_floats(*cfg))
        if n < 0:
            raise ValueError("the mel basis needs sr > 0, 1 <= n_mels <= 1024 and 0 <= fmin < fmax <= sr / 2 (got sr=%r, n_mels=%r, "
                             "fmin=%r, fmax=%r)" % (sr, n_mels, fmin, fmax))
        host = np.zeros(n, dtype=np.float32)
        _lib.check(L.mla_melspec_build_band_tables(*cfg, host.ctypes.data_as(ctypes.c_void_p)))
        _melspec_tables[key] = torch.from_numpy(host).to(device)
    return _melspec_tables[key]


def melspec_frames_librosa(n_samples, hop_length):
    """Spectrogram columns without padding (center=False): 1 + (n_samples - 2048) // hop_length; -1 below one whole frame."""
    return int(_lib.lib().mla_melspec_nopad_frames(int(n_samples), int(hop_length)))


def _check_nopad(n, hop_length):
    if n < 2048:
        raise ValueError("without padding (center=False) a clip needs at least 2048 samples, one whole frame (got %d)" % n)
    if int(hop_length) < 1:
        raise ValueError("hop_length must be a positive integer (got %r)" % (hop_length,))


def melspec_db_unclipped_librosa(pcm, sr, n_mels, hop_length, fmin=0.0, fmax=None, htk=False):
    """melspec_db_unclipped on UNPADDED frames (librosa's center=False) with the mel basis (fmin, fmax, htk): (clips, n) device PCM
    -> ((clips, n_mels, 1 + (n - 2048) // hop_length) dB values before the top_db clip, the workspace of per-clip partial maxima that
    melspec_bags reads). Kernel 1 of the VGGish branch's librosa path (csrc/melspec.hip, melspec_nopad_db_kernel)."""
    assert pcm.dim() == 2 and pcm.is_cuda and pcm.dtype == torch.float32 and (pcm.shape[1] <= 1 or pcm.stride(1) == 1)
    clips, n = pcm.shape
    _check_nopad(n, hop_length)
    L = _lib.lib()
    tab = melspec_band_tables(pcm.device, sr, n_mels, fmin, float(sr) / 2 if fmax is None else fmax, htk)
    ws = torch.empty(int(L.mla_melspec_nopad_workspace_bytes(clips, n, int(hop_length))) // 4, dtype=torch.float32, device=pcm.device)
    db = torch.empty((clips, int(n_mels), melspec_frames_librosa(n, hop_length)), dtype=torch.float32, device=pcm.device)
    vp = ctypes.c_void_p
    from . import ops
    _lib.check(ops._timed("melspec_nopad_db", L.mla_melspec_nopad_db, vp(pcm.data_ptr()), clips, n, pcm.stride(0) if clips > 1 else n,
                          int(hop_length), int(n_mels), MELSPEC_AMIN, vp(tab.data_ptr()), tab.shape[0], vp(db.data_ptr()), vp(ws.data_ptr()),
                          _lib.stream_ptr()))
    return db, ws


def melspec_bags(db, ws, n_samples, hop_length, top_db, n_images, image_w, image_stride, out_dtype=torch.float32):
    """melspec_images for the spectrogram and workspace of melspec_db_unclipped_librosa, written in `out_dtype` (float32, or
    bfloat16 by one rounding to nearest even): (clips, n_mels, frames) -> (clips, n_images, 1, n_mels, image_w). Kernel 2 of the
    VGGish branch's librosa path: a select and a gather, bit-determined by `db`."""
    clips, n_mels, _ = db.shape
    _check_nopad(int(n_samples), hop_length)
    out_code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}[out_dtype]
    out = torch.empty((clips, int(n_images), 1, n_mels, int(image_w)), dtype=out_dtype, device=db.device)
    vp = ctypes.c_void_p
    from . import ops
    _lib.check(ops._timed("melspec_nopad_bags", _lib.lib().mla_melspec_nopad_bags, vp(db.data_ptr()), vp(ws.data_ptr()), clips,
                          int(n_samples), int(hop_length), n_mels, float(top_db), int(n_images), int(image_w), int(image_stride),
                          vp(out.data_ptr()), out_code, _lib.stream_ptr()))
    return out


def melspectrogram_db(pcm, sr, n_mels, hop_length, top_db=80.0, center=True, htk=False, fmin=0.0, fmax=None):
    """librosa.power_to_db(librosa.feature.melspectrogram(y, sr=sr, n_mels=n_mels, hop_length=hop_length), top_db=top_db) with
    librosa's defaults (n_fft 2048, periodic Hann, centre reflect padding, power 2, Slaney mel basis; ref 1.0, amin 1e-10) for
    every row of `pcm`: (clips, n) float32 device PCM -> (clips, n_mels, 1 + n // hop_length) float32. top_db=None skips the clip.
    Clips shorter than 1025 samples raise ValueError (reflect padding by 1024 needs them).

    center=False is librosa's unpadded framing, (clips, n_mels, 1 + (n - 2048) // hop_length) from 2048 samples on, and takes the
    mel basis of melspectrogram's htk / fmin / fmax keywords (fmax None: sr / 2) -- the VGGish branch's librosa path is
    (16000, 64, 160, center=False, htk=True, fmin=125, fmax=7500). With center=True only the default basis is built."""
    if not center:
        if top_db is not None and top_db < 0:
            raise ValueError("top_db must be non-negative")
        db, ws = melspec_db_unclipped_librosa(pcm, sr, n_mels, hop_length, fmin, fmax, htk)
        if top_db is None:
            return db
        return melspec_bags(db, ws, pcm.shape[1], hop_length, top_db, 1, db.shape[2], 0)[:, 0, 0]
    if htk or fmin != 0.0 or (fmax is not None and float(fmax) != float(sr) / 2):
        raise NotImplementedError("the centred spectrogram is built with librosa's default mel basis only (htk=False, fmin=0, fmax=sr/2); "
                                  "another basis runs with center=False")
    if pcm.shape[1] < 1025:
        raise ValueError("melspectrogram_db needs at least 1025 samples per clip (got %d)" % pcm.shape[1])
    if top_db is not None and top_db < 0:
        raise ValueError("top_db must be non-negative")
    db, ws = melspec_db_unclipped(pcm, sr, n_mels, hop_length)
    if top_db is None:
        return db
    return melspec_images(db, ws, pcm.shape[1], hop_length, top_db, 1, db.shape[2], 0)[:, 0, 0]


def _as_device_signal(signal):
    dev = _device()
    if isinstance(signal, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(signal.astype(np.float32))).to(dev)
    return signal.to(dev).float().contiguous()


def stft_magnitude(signal, fft_length, hop_length, window_length):
    """mel_features.stft_magnitude (mel_features.py:71-92) on the GPU for any window / hop and
    power-of-two fft_length <= 4096: (frames, fft_length/2 + 1) float32 CUDA tensor."""
    from .torchvggish import mel_features
    x = _as_device_signal(signal)
    assert x.dim() == 1
    n = x.shape[0]
    frames = 1 + int(np.floor((n - window_length) / hop_length))
    if frames < 0:
        raise ValueError("negative dimensions are not allowed")
    bins = fft_length // 2 + 1
    out = torch.empty((frames, bins), dtype=torch.float32, device=x.device)
    if frames == 0:
        return out
    window = torch.from_numpy(mel_features.periodic_hann(window_length).astype(np.float32)).to(x.device)
    m = np.arange(fft_length // 2)
    tw = np.stack([np.cos(2 * np.pi * m / fft_length), -np.sin(2 * np.pi * m / fft_length)], axis=1).astype(np.float32)
    tw = torch.from_numpy(np.ascontiguousarray(tw)).to(x.device)
    vp = ctypes.c_void_p
    _lib.check(_lib.lib().mla_stft_magnitude(vp(x.data_ptr()), n, vp(window.data_ptr()), vp(tw.data_ptr()), int(window_length),
                                             int(hop_length), int(fft_length), vp(out.data_ptr()), _lib.stream_ptr()))
    return out


def log_mel_spectrogram(data, audio_sample_rate, log_offset, window_length_secs, hop_length_secs, **kwargs):
    """mel_features.log_mel_spectrogram (mel_features.py:192-223) on the GPU for any configuration:
    (frames, num_mel_bins) float32 CUDA tensor. The mel matrix is host-side setup, as in the reference."""
    from .torchvggish import mel_features
    win = int(round(audio_sample_rate * window_length_secs))
    hop = int(round(audio_sample_rate * hop_length_secs))
    fft = 2 ** int(np.ceil(np.log(win) / np.log(2.0)))
    spec = stft_magnitude(data, fft, hop, win)
    mel = mel_features.spectrogram_to_mel_matrix(num_spectrogram_bins=spec.shape[1], audio_sample_rate=audio_sample_rate, **kwargs)
    melt = torch.from_numpy(np.ascontiguousarray(mel.astype(np.float32))).to(spec.device)
    out = torch.empty((spec.shape[0], mel.shape[1]), dtype=torch.float32, device=spec.device)
    vp = ctypes.c_void_p
    _lib.check(_lib.lib().mla_mel_log(vp(spec.data_ptr()), vp(melt.data_ptr()), spec.shape[0], spec.shape[1], mel.shape[1],
                                      float(log_offset), vp(out.data_ptr()), _lib.stream_ptr()))
    return out
