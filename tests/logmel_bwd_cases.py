"""Shared by test_logmel_bwd_cpu.py and test_logmel_bwd_gpu.py (no GPU needed here): the inputs of the log-mel backward tests, the
float64 reference -- torch autograd through unfold / rfft(n=512) / abs / matmul / log with the window and the mel matrix of
mla_logmel_reference_tables -- and the same restated in float32 on the CPU, the yardstick for what float32 arithmetic costs on a
case. Every reference is computed once per process and handed out read-only.

The function is ill-conditioned where a bin's magnitude A_k sinks into the frame's rounding noise (X_k / A_k is a unit phasor, and
1 / (mel + 0.01) amplifies up to 100 x): a pure sine has bins at 1e-17 of its peak and a float32 restatement is then 38 % off in
l2. That belongs to the function, not to a kernel, so every case here keeps its least A_k / max A over the used bins above 1e-5
(asserted in test_logmel_bwd_cpu.py)."""

import ctypes
import functools
import importlib

import numpy as np
import torch

from conftest import PKG

HOP, WIN, FFT, BANDS, EX = 160, 400, 512, 64, 96
ITEM_CHUNKS, MAX_WG = 14, 512                 # the kernel's work item (hop-chunks) and grid cap (csrc/logmel_bwd_core.h)
YARDSTICK_FACTOR = 16                         # err(kernel) <= 16 x err(float32 restatement): four bits over another f32 transform


def counts(n):
    frames = 1 + (n - WIN) // HOP if n >= WIN else 0
    return frames, max(frames // EX, 0)


def items_per_row(n):
    return -(-(-(-n // HOP)) // ITEM_CHUNKS)


def cap_crossing_shape():
    """The smallest (W, 160 000) at which a workgroup takes a second item."""
    ipr = items_per_row(160000)
    return MAX_WG // ipr + 1, 160000


@functools.lru_cache(maxsize=None)
def tables():
    """(window (400,), mel (257, 64)) float64, from the library."""
    L = importlib.import_module(PKG + "._lib").lib()
    win, mel = np.zeros(WIN), np.zeros((FFT // 2 + 1, BANDS))
    assert L.mla_logmel_reference_tables(win.ctypes.data_as(ctypes.c_void_p), mel.ctypes.data_as(ctypes.c_void_p)) == 0
    # the reference is only a reference for the kernel if this is the matrix the kernel's transposed mel step was built from:
    # every non-zero of it must be one of the <= 2 weights per bin of the backward table
    btab = np.zeros(int(L.mla_logmel_bwd_table_floats()), dtype=np.float32)
    assert L.mla_logmel_bwd_build_tables(btab.ctypes.data_as(ctypes.c_void_p)) == 0
    assert int(np.count_nonzero(btab[1:1024:4]) + np.count_nonzero(btab[2:1024:4])) == int(np.count_nonzero(mel))
    return torch.from_numpy(win), torch.from_numpy(mel)


def _noise(seed, shape, scale=1.0):
    return (scale * np.random.default_rng(seed).uniform(-1.0, 1.0, shape)).astype(np.float32)


def _sine_mix(n=15600):
    t = np.arange(n, dtype=np.float64)
    return (0.5 * np.sin(2 * np.pi * 1000.0 * t / 16000.0) + 0.05 * np.random.default_rng(15).uniform(-1.0, 1.0, n)).astype(np.float32)


def _grad_out(seed, rows, n):
    return np.random.default_rng(1000 + seed).standard_normal((rows * counts(n)[1], EX, BANDS)).astype(np.float32)


def _case_g():
    n = 30960
    pcm = np.zeros((3, n), dtype=np.float32)
    pcm[0] = _noise(13, (1, n))[0]
    pcm[1, :15600] = _sine_mix()
    return pcm


_MAKERS = {
    "a": lambda: _noise(11, (1, 15600)),
    "b": lambda: _noise(12, (1, 30959)),
    "c": lambda: _noise(13, (1, 30960)),
    "d": lambda: _noise(14, (1, 15600), 1e-3),
    "e": lambda: _sine_mix()[None],
    "f": lambda: np.random.default_rng(16).integers(-32768, 32768, (1, 15600)).astype(np.int16),
    "g": _case_g,
    "cap": lambda: _noise(17, cap_crossing_shape()),
}
CASES = ("a", "b", "c", "d", "e", "f", "g")
CONDITIONED = ("a", "b", "c", "d", "e", "f")
STRIDE_PAD = {"g": 37}                         # case g's rows lie n + 37 elements apart


@functools.lru_cache(maxsize=None)
def case(name):
    """(pcm (W, n) float32 or int16 tensor, G (W * N, 96, 64) float32 tensor); read-only."""
    pcm = _MAKERS[name]()
    g = _grad_out(sorted(_MAKERS).index(name), pcm.shape[0], pcm.shape[1])
    return torch.from_numpy(pcm), torch.from_numpy(g)


def as_float(pcm, dtype):
    return pcm.to(dtype) / 32768 if pcm.dtype == torch.int16 else pcm.to(dtype)


def forward(x, dtype):
    """x (W, n) of `dtype` -> (out (W, 96 N, 64), |X| (W, 96 N, 257)); differentiable."""
    win, mel = (t.to(dtype) for t in tables())
    used = counts(x.shape[1])[1] * EX
    if used == 0:
        z = x.sum() * 0
        return z.expand(x.shape[0], 0, BANDS), z.expand(x.shape[0], 0, FFT // 2 + 1)
    frames = x[:, :HOP * (used - 1) + WIN].unfold(-1, WIN, HOP) * win
    mag = torch.fft.rfft(frames, n=FFT).abs()
    return torch.log(mag @ mel + 0.01), mag


def autograd_grad(pcm, g, dtype):
    x = as_float(pcm, dtype).clone().requires_grad_(True)
    out, _ = forward(x, dtype)
    (out * g.to(dtype).view(out.shape)).sum().backward()
    return x.grad.detach()


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 d L / d wave (W, n) for L = sum(out * G)."""
    pcm, g = case(name)
    return autograd_grad(pcm, g, torch.float64)


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """err of the float32 CPU restatement on the case."""
    pcm, g = case(name)
    return err(autograd_grad(pcm, g, torch.float32), reference(name))


def err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def bound(name):
    return YARDSTICK_FACTOR * yardstick(name)


def loop_form(pcm, g):
    """The formulas of the issue, frame by frame in float64 with explicit cos / sin sums -> (W, n)."""
    win, mel = tables()
    x = as_float(pcm, torch.float64)
    n_wave, n = x.shape
    used = counts(n)[1] * EX
    k, m = torch.arange(FFT // 2 + 1, dtype=torch.float64), torch.arange(WIN, dtype=torch.float64)
    ang = 2 * np.pi / FFT * torch.outer(k, m)
    cos, sin = torch.cos(ang), torch.sin(ang)
    gg = g.double().view(n_wave, used, BANDS)
    dx = torch.zeros_like(x)
    for w in range(n_wave):
        for f in range(used):
            y = win * x[w, HOP * f:HOP * f + WIN]
            xr, xi = cos @ y, -(sin @ y)
            a = torch.sqrt(xr * xr + xi * xi)
            da = mel @ (gg[w, f] / (a @ mel + 0.01))
            safe = torch.where(a > 0, a, torch.ones_like(a))
            ur = torch.where(a > 0, da * xr / safe, torch.zeros_like(a))
            ui = torch.where(a > 0, da * xi / safe, torch.zeros_like(a))
            dx[w, HOP * f:HOP * f + WIN] += win * (ur @ cos - ui @ sin)
    return dx


def least_relative_magnitude(name):
    """min A_k / max A over the used frames and bins 5 .. 239, float64."""
    pcm, _ = case(name)
    with torch.no_grad():
        _, mag = forward(as_float(pcm, torch.float64), torch.float64)
    return float(mag[..., 5:240].min() / mag.max())
