"""float64 numpy restatement of the librosa (< 0.10) calls behind the reference's ResNet images (dataset.py:309-316, :329-363):

    librosa.feature.melspectrogram(y, sr=sr, n_mels=n_mels, hop_length=hop)      # n_fft = win_length = 2048, periodic Hann,
                                                                                 # center=True, pad_mode="reflect", power=2,
                                                                                 # filters.mel(htk=False, norm="slaney", fmin=0, fmax=sr/2)
    librosa.power_to_db(S)                                                       # ref=1.0, amin=1e-10, top_db=80.0
    split(spec, T, 224, 224, overlap)

written from librosa's published definitions; librosa itself is not a test dependency and parity with it is NOT pinned
(DESIGN.md section 5). The documented values its own docstrings give for the mel scale anchor this file in
tests/test_melspec_cpu.py. Also here: the seeded test waveforms, an independent float32 evaluation of the same formulas (the
tolerance baseline) and the power-domain closeness measure shared by the CPU and GPU tests.
"""

import numpy as np
import scipy.fft

N_FFT = 2048
AMIN = 1e-10
TOP_DB = 80.0


def hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_frequencies(n_mels=128, fmin=0.0, fmax=11025.0):
    return mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels))


def mel_filters(sr, n_mels, n_fft=N_FFT):
    """(n_mels, 1 + n_fft // 2) Slaney-normalised triangular filterbank."""
    fftfreqs = np.linspace(0, float(sr) / 2, 1 + n_fft // 2)
    mel_f = mel_frequencies(n_mels + 2, 0.0, float(sr) / 2)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    w = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        w[i] = np.maximum(0, np.minimum(lower, upper))
    return w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def hann_periodic(n=N_FFT):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def num_frames(n, hop):
    return 1 + n // hop


def frame_matrix(y, hop, dtype=np.float64):
    """(frames, 2048) windowed frames of the centre-padded (reflect) signal."""
    y = np.asarray(y, dtype=dtype)
    assert y.ndim == 1 and len(y) > N_FFT // 2
    padded = np.pad(y, N_FFT // 2, mode="reflect")
    idx = np.arange(num_frames(len(y), hop))[:, None] * hop + np.arange(N_FFT)[None, :]
    return padded[idx] * hann_periodic().astype(dtype)


def mel_power(y, sr, n_mels, hop):
    """S = mel @ |STFT|^2, float64, shape (n_mels, frames)."""
    spec = np.fft.rfft(frame_matrix(y, hop), axis=1)
    power = spec.real ** 2 + spec.imag ** 2
    return mel_filters(sr, n_mels) @ power.T


def power_to_db(S, amin=AMIN, top_db=TOP_DB):
    D = 10.0 * np.log10(np.maximum(amin, S))
    return D if top_db is None else np.maximum(D, D.max() - top_db)


def melspectrogram_db(y, sr, n_mels, hop, top_db=TOP_DB):
    return power_to_db(mel_power(y, sr, n_mels, hop), top_db=top_db)


def hop_length(samples_num, x_size, overlap, T=10):
    return samples_num // (x_size * 4) if overlap else samples_num // (x_size * T)


def split_step(width, num_frames_, frame_length, overlap):
    return (width - frame_length) // (num_frames_ - 1) if overlap else frame_length


def split(spec, num_frames_, frame_length, overlap):
    step = split_step(spec.shape[1], num_frames_, frame_length, overlap)
    frames = np.array([spec[:, i:i + frame_length] for i in range(0, spec.shape[1], step)][:num_frames_])
    assert frames.shape == (num_frames_, spec.shape[0], frame_length), frames.shape
    return frames


# ---- the tolerance baseline: the same formulas evaluated independently in float32 ------------------------------------------

def mel_power_f32(y, sr, n_mels, hop):
    """scipy.fft.rfft (pocketfft, float32 in -> complex64 out), power and mel product in float32, and the float32 dB round trip
    S -> 10 log10(max(amin, S)) -> 10^(D/10) that any float32 dB output goes through. Returns float64 values of float32 results."""
    fr = frame_matrix(np.asarray(y, dtype=np.float32), hop, dtype=np.float32)
    spec = scipy.fft.rfft(fr, axis=1)
    assert spec.dtype == np.complex64
    power = spec.real * spec.real + spec.imag * spec.imag
    mel = mel_filters(sr, n_mels).astype(np.float32)
    S = np.zeros((n_mels, power.shape[0]), dtype=np.float32)
    for k in range(power.shape[1]):            # ascending bins, one rounding per product and per sum: no BLAS, so the same everywhere
        S += mel[:, k, None] * power[None, :, k]
    assert S.dtype == np.float32
    D = (np.float32(10.0) * np.log10(np.maximum(np.float32(AMIN), S))).astype(np.float32)
    return db_to_power(D)


def db_to_power(D):
    return 10.0 ** (np.asarray(D, dtype=np.float64) / 10.0)


def power_errors(S, S_ref, amin=AMIN):
    """Per-element |S - S_ref| after max(amin, .) on the reference, the reference and its per-frame strongest band."""
    r = np.maximum(amin, np.asarray(S_ref, dtype=np.float64))
    g = np.maximum(amin, np.asarray(S, dtype=np.float64))
    return np.abs(g - r), r, r.max(axis=0, keepdims=True)


def baseline_constants(pairs):
    """(rel, floor) of the form |S - S_ref| <= rel * S_ref + floor * max_band(S_ref of the frame) that the given (S, S_ref) pairs
    just meet: rel is the worst relative error among the elements within 30 dB of their frame's strongest band (where the floor
    term is negligible), floor the worst remaining error relative to the frame's strongest band."""
    rel = floor = 0.0
    for S, S_ref in pairs:
        err, r, top = power_errors(S, S_ref)
        strong = r >= 1e-3 * top
        rel = max(rel, float((err[strong] / r[strong]).max()))
    for S, S_ref in pairs:
        err, r, top = power_errors(S, S_ref)
        floor = max(floor, float((np.maximum(err - rel * r, 0.0) / top).max()))
    return rel, floor


def power_close(S, S_ref, rel, floor):
    """(ok, worst ratio error / bound) of the project's mel-domain form (tests/test_abi_cpu.py mel_domain_close) on powers."""
    err, r, top = power_errors(S, S_ref)
    bound = rel * r + floor * top
    ratio = err / bound
    return bool(np.all(err <= bound)), float(ratio.max())


# ---- seeded waveforms (no files) ---------------------------------------------------------------------------------------------

WAVEFORMS = ("noise", "chirp", "tones", "burst", "silence")


def waveform(name, n, sr=22050, seed=0):
    rng = np.random.default_rng([seed, WAVEFORMS.index(name), n])
    t = np.arange(n) / float(sr)
    if name == "noise":
        x = rng.uniform(-0.5, 0.5, n)
    elif name == "chirp":                      # 100 Hz -> 8 kHz, linear in time
        dur = n / float(sr)
        x = 0.5 * np.sin(2 * np.pi * (100.0 * t + 0.5 * (8000.0 - 100.0) / dur * t * t))
    elif name == "tones":                      # steady tones at 0 / -30 / -60 dB
        x = 0.5 * (np.sin(2 * np.pi * 440.0 * t) + 10 ** (-30 / 20.0) * np.sin(2 * np.pi * 2500.0 * t + 1.0)
                   + 10 ** (-60 / 20.0) * np.sin(2 * np.pi * 7000.0 * t + 2.0))
    elif name == "burst":                      # a loud 50 ms burst over quiet noise whose level rises by 60 dB along the clip,
        x = 10.0 ** (-5.0 + 3.0 * np.arange(n) / n) * rng.standard_normal(n)      # so that the top_db floor cuts through it
        b0 = n // 3
        bn = min(int(0.05 * sr), n - b0)
        x[b0:b0 + bn] += 0.8 * np.sin(2 * np.pi * 1000.0 * t[:bn]) * np.hanning(bn)
    elif name == "silence":
        x = np.zeros(n)
    else:
        raise KeyError(name)
    return x.astype(np.float32)
