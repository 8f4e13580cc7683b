"""float64 numpy restatement of the librosa (< 0.10) calls behind the reference's VGGish bags on the librosa path
(dataset.py:232-243, :305-307, :316, :342-359):

    librosa.feature.melspectrogram(y, sr=16000, n_mels=64, hop_length=160, center=False, htk=True, fmin=125, fmax=7500)
                                                     # n_fft = win_length = 2048, periodic Hann, power=2, NO padding: frame f is
                                                     # y[160 f : 160 f + 2048]; filters.mel(htk=True, norm="slaney")
    librosa.power_to_db(S)                           # ref=1.0, amin=1e-10, top_db=80.0
    split(spec, 10, 96, 64, overlap=True)

written from librosa's published definitions, like tests/librosa_restated.py, whose shared pieces (window, power_to_db, split,
the waveforms, the float32 baseline's measure and the power-domain closeness) it imports; librosa itself is not a test dependency
and parity with it is NOT pinned.
"""

import numpy as np
import scipy.fft

import librosa_restated as R
from librosa_restated import AMIN, N_FFT, TOP_DB, WAVEFORMS, baseline_constants, db_to_power, hann_periodic, power_close, power_to_db, split, split_step, waveform  # noqa: F401

SR, N_MELS, HOP, FMIN, FMAX = 16000, 64, 160, 125.0, 7500.0
N_CLIP = 64000


def hz_to_mel(f):
    """HTK scale (librosa hz_to_mel(htk=True))."""
    return 2595.0 * np.log10(1.0 + np.asanyarray(f, dtype=np.float64) / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asanyarray(m, dtype=np.float64) / 2595.0) - 1.0)


def mel_frequencies(n_mels, fmin, fmax):
    return mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels))


def mel_filters(sr=SR, n_mels=N_MELS, fmin=FMIN, fmax=FMAX, n_fft=N_FFT):
    """(n_mels, 1 + n_fft // 2) triangular filterbank on the HTK scale, Slaney area normalisation (librosa's default norm)."""
    fftfreqs = np.linspace(0, float(sr) / 2, 1 + n_fft // 2)
    mel_f = mel_frequencies(n_mels + 2, fmin, fmax)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    w = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        w[i] = np.maximum(0, np.minimum(lower, upper))
    return w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def num_frames(n, hop=HOP):
    """center=False: whole frames only."""
    return 1 + (n - N_FFT) // hop


def frame_matrix(y, hop=HOP, dtype=np.float64):
    """(frames, 2048) windowed frames of the unpadded signal."""
    y = np.asarray(y, dtype=dtype)
    assert y.ndim == 1 and len(y) >= N_FFT
    idx = np.arange(num_frames(len(y), hop))[:, None] * hop + np.arange(N_FFT)[None, :]
    return y[idx] * hann_periodic().astype(dtype)


def mel_power(y, hop=HOP, mel=None):
    """S = mel @ |STFT|^2, float64, shape (n_mels, frames)."""
    spec = np.fft.rfft(frame_matrix(y, hop), axis=1)
    power = spec.real ** 2 + spec.imag ** 2
    return (mel_filters() if mel is None else mel) @ power.T


def melspectrogram_db(y, hop=HOP, top_db=TOP_DB, mel=None):
    return power_to_db(mel_power(y, hop, mel), top_db=top_db)


def mel_power_f32(y, hop=HOP, mel=None):
    """The tolerance baseline of librosa_restated.mel_power_f32 on this variant's frames and filterbank: pocketfft on float32
    frames, float32 power, mel product and dB round trip. Returns float64 values of float32 results."""
    fr = frame_matrix(np.asarray(y, dtype=np.float32), hop, dtype=np.float32)
    spec = scipy.fft.rfft(fr, axis=1)
    assert spec.dtype == np.complex64
    power = spec.real * spec.real + spec.imag * spec.imag
    mel = (mel_filters() if mel is None else mel).astype(np.float32)
    S = np.zeros((mel.shape[0], power.shape[0]), dtype=np.float32)
    for k in range(power.shape[1]):            # ascending bins, one rounding per product and per sum
        S += mel[:, k, None] * power[None, :, k]
    assert S.dtype == np.float32
    D = (np.float32(10.0) * np.log10(np.maximum(np.float32(AMIN), S))).astype(np.float32)
    return db_to_power(D)


def clip_waveform(name, n):
    """R.waveform with its default sr argument, read at 16 kHz: the chirp sweeps 73 -> 5 805 Hz and the tones sit at 319, 1 814 and
    5 079 Hz, all inside the 125 .. 7 500 Hz passband."""
    return R.waveform(name, n)
