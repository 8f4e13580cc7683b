"""NaN samples through the front-ends' lane code on the CPU: the host simulations of the existing *_cpu.py tests (built by their
fixtures from csrc/*_hostsim.cpp, which compile the very headers the kernels include) against the float64 restatements, by the rule of
tests/nonfinite_cases.py -- a frame that reads the NaN sample is NaN in every band, as np.maximum(amin, .) and the reference's
log leave it; every other frame keeps the clean run's bits and with them the finite tests' tolerance. Also the host form of
csrc/nanprop.h itself, which these simulations (and nothing on the GPU) run."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import librosa_htk_restated as H
import librosa_restated as R
from conftest import PKG, ROOT
from nonfinite_cases import frames_touching, nan_sample
from oracle import dataset_frames as ods
from test_logmel_bags_cpu import LENGTHS, ROW, hostsim as bags_hostsim, noise, rows_and_counts     # noqa: F401 (fixtures)
from test_melspec_cpu import FLOOR, REL, SR, hostsim as melspec_hostsim, run_hostsim as run_melspec   # noqa: F401
from test_melspec_htk_cpu import hostsim as wave_hostsim, run_hostsim as run_wave                    # noqa: F401


def check_spectrogram(D, clean, ref_power, touched, what):
    """D, clean: (bands, frames) dB of the poisoned and the clean clip; ref_power: float64 powers of the poisoned clip."""
    nan = np.isnan(ref_power)
    assert np.array_equal(nan, np.broadcast_to(touched[None, :], nan.shape)) and touched.any() and not touched.all(), what
    assert np.array_equal(np.isnan(D), nan), "%s: %d of %d NaN elements came out finite" % (what, int((nan & ~np.isnan(D)).sum()), int(nan.sum()))
    assert not np.isinf(D).any()
    assert np.array_equal(D[:, ~touched].view(np.int32), clean[:, ~touched].view(np.int32)), what + ": a frame without the sample changed"
    assert R.power_close(R.db_to_power(D[:, ~touched]), ref_power[:, ~touched], REL, FLOOR)[0], what


@pytest.mark.parametrize("n,hop,n_mels", [(5000, 98, 224), (4096, 128, 32)])
def test_melspec_host_simulation_keeps_a_nan_sample(melspec_hostsim, n, hop, n_mels):
    """melspec_core.h (centre padding, reflect): the first and the last sample are read twice by the frames at the ends."""
    x = R.waveform("noise", n)
    clean = run_melspec(melspec_hostsim, x, hop, n_mels)
    for index in (0, n // 2, n - 1):
        bad = nan_sample(x, index)
        ref = R.mel_power(bad, SR, n_mels, hop)
        touched = np.isnan(R.frame_matrix(bad, hop)).any(axis=1)
        assert touched.sum() >= frames_touching(index, len(touched), hop, R.N_FFT, pad=R.N_FFT // 2).sum()
        check_spectrogram(run_melspec(melspec_hostsim, bad, hop, n_mels), clean, ref, touched, "melspec n=%d hop=%d sample %d" % (n, hop, index))


@pytest.mark.parametrize("n", [4608, 5088])
def test_melspec_wave_host_simulation_keeps_a_nan_sample(wave_hostsim, n):
    """melspec_wave_core.h (no padding, HTK basis): one frame past a 16-frame run, and twenty frames."""
    x = H.clip_waveform("noise", n)
    clean = run_wave(wave_hostsim, x)
    for index in (0, n // 2, H.N_FFT + (H.num_frames(n) - 1) * H.HOP - 1):
        bad = nan_sample(x, index)
        touched = frames_touching(index, H.num_frames(n), H.HOP, H.N_FFT)
        check_spectrogram(run_wave(wave_hostsim, bad), clean, H.mel_power(bad), touched, "melspec (no padding) n=%d sample %d" % (n, index))


@pytest.mark.parametrize("n_frames,stride", [(10, 32), (4, 96)])
def test_logmel_bags_host_simulation_keeps_a_nan_sample(bags_hostsim, n_frames, stride):
    """logmel_bags_core.h: one NaN sample in the row of 30 960 samples (two examples). Its row is NaN where the float64 chain
    split(create_spec_native(x)) is; every other row, and the rest of its own, keep the clean run's bits."""
    rows, counts = rows_and_counts()
    B, i = len(LENGTHS), LENGTHS.index(30960)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                                  # noqa: E731
    outs = []
    bad = nan_sample(rows, (i, 20000))
    for r in (rows, bad):
        out, writes = np.full((B, n_frames, 64, 96), 7.0, dtype=np.float32), np.zeros((B, n_frames, 64, 96), dtype=np.int32)
        assert bags_hostsim.hostsim_logmel_bags(p(r), B, ROW, ROW, p(counts), n_frames, stride, p(out), p(writes)) == 0
        outs.append(out)
    clean, got = outs
    ref = np.asarray(ods.split(ods.create_spec_native(bad[i, :30960].astype(np.float64)), 10, 96, 64, stride == 32))
    nan = np.isnan(ref)
    assert nan.any() and not nan.all() and np.isfinite(clean).all()
    assert np.array_equal(np.isnan(got[i]), nan) and not np.isnan(np.delete(got, i, axis=0)).any() and not np.isinf(got).any()
    keep = ~np.isnan(got)
    assert np.array_equal(got[keep].view(np.int32), clean[keep].view(np.int32))


NANPROP_PROBE = r"""
#include "nanprop.h"
extern "C" void probe(const float* a, const float* b, int n, float* mx, float* mn, float* relu) {
    for (int i = 0; i < n; ++i) { mx[i] = mla::nan_max(a[i], b[i]); mn[i] = mla::nan_min(a[i], b[i]); relu[i] = mla::nan_relu(a[i]); }
}
extern "C" float pool(float a, float b, float c, float d) { return mla::nan_pool_relu(a, b, c, d); }
"""


def test_nanprop_host_form_is_the_ieee_2019_maximum(tmp_path):
    """csrc/nanprop.h as the host simulations compile it: NaN from either side, +0 over -0 (what v_maximum3_f32 returns on the device),
    infinities ordered -- against np.maximum / np.minimum, bit for bit."""
    src, so = tmp_path / "probe.cpp", tmp_path / "probe.so"
    src.write_text(NANPROP_PROBE)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, PKG, "csrc"), "-o", str(so), str(src)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.pool.restype = ctypes.c_float
    lib.pool.argtypes = [ctypes.c_float] * 4
    vals = np.array([np.nan, -np.inf, -1.5, -0.0, 0.0, 2.0 ** -149, 3.0, np.inf], dtype=np.float32)
    a, b = (np.ascontiguousarray(v.reshape(-1)) for v in np.meshgrid(vals, vals))
    out = [np.zeros_like(a) for _ in range(3)]
    p = lambda t: t.ctypes.data_as(ctypes.c_void_p)                                                  # noqa: E731
    lib.probe(p(a), p(b), len(a), *[p(o) for o in out])
    zero = (a == 0) & (b == 0)
    want_max = np.where(zero, np.where(np.signbit(a) & np.signbit(b), np.float32(-0.0), np.float32(0.0)), np.maximum(a, b))
    want_min = np.where(zero, np.where(np.signbit(a) | np.signbit(b), np.float32(-0.0), np.float32(0.0)), np.minimum(a, b))
    nan = np.isnan(a) | np.isnan(b)
    for got, want in ((out[0], want_max), (out[1], want_min)):
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32))
    relu = out[2]
    assert np.array_equal(np.isnan(relu), np.isnan(a)) and np.array_equal(relu[~np.isnan(a)].view(np.int32), np.maximum(a, np.float32(0))[~np.isnan(a)].view(np.int32) & 0x7fffffff)
    assert np.isnan(lib.pool(1.0, 2.0, float("nan"), 3.0)) and lib.pool(-1.0, -2.0, -np.inf, -3.0) == 0.0 and lib.pool(1.0, np.inf, 0.0, 2.0) == np.inf
