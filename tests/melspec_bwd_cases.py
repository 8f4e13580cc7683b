"""Shared by test_melspec_bwd_cpu.py and test_melspec_bwd_gpu.py (no GPU needed here): the inputs of the mel-dB backward tests, the
float64 reference -- torch autograd through pad(reflect) / unfold / rfft / re^2 + im^2 / matmul / 10 log10(clamp(., amin)) /
maximum(D, D.max() - top_db) / the split, with the window and the Slaney basis of mla_melspec_build_tables -- the same restated in
float32 on the CPU (the yardstick for what float32 arithmetic costs on a case), and the formulas of DESIGN.md 3.17 as explicit
float64 loops. Every reference is computed once per process and handed out read-only.

The top_db floor makes the function discontinuous in two places: a cell that crosses the floor switches its gradient off, and the
cell that holds the maximum collects the floor's own gradient. A case is therefore only a case for a float32 kernel if (a) its
maximum is unique by >= 0.01 dB and (b) no cell lies within `margin` of the floor, where margin >= 16 x the float32 restatement's
largest dB error over the cells within 1 dB of the floor (conditioning(), asserted in test_melspec_bwd_cpu.py). That is a
condition of the inputs, checked in float64 on the CPU; it is not a tolerance on the kernel."""

import ctypes
import functools
import importlib
from collections import namedtuple

import numpy as np
import torch

from conftest import PKG
from logmel_bwd_cases import YARDSTICK_FACTOR  # err(kernel) <= 16 x err(float32 restatement): four bits over another f32 transform

FFT, PAD, BINS = 2048, 1024, 1025
SR = 22050
AMIN = float(np.float32(1e-10))
TOP_DB = 80.0
RUN_FRAMES = 32                                # frames per workgroup of melspec_db_bwd_kernel (csrc/melspec_bwd_core.h)
MIN_MAX_GAP_DB, MARGIN_FACTOR, NEAR_DB = 0.01, 16, 1.0

Case = namedtuple("Case", "pcm g hop n_mels n_images image_w stride floor_grad")


def frames_of(n, hop):
    return 1 + n // hop


@functools.lru_cache(maxsize=None)
def tables(n_mels):
    """(window (2048,), mel (n_mels, 1025)) float64: the float32 tables of the library, which are what the kernels multiply by."""
    L = importlib.import_module(PKG + "._lib").lib()
    n = int(L.mla_melspec_table_floats(float(SR), n_mels))
    tab = np.zeros(n, dtype=np.float32)
    assert L.mla_melspec_build_tables(float(SR), n_mels, tab.ctypes.data_as(ctypes.c_void_p)) == 0
    meta = tab[FFT + 2 * 1536:FFT + 2 * 1536 + 3 * n_mels].view(np.int32).reshape(n_mels, 3)
    weights = tab[FFT + 2 * 1536 + 3 * n_mels:]
    mel = np.zeros((n_mels, BINS))
    for b, (first, bins, off) in enumerate(meta):
        mel[b, first:first + bins] = weights[off:off + bins]
    assert ((mel != 0).sum(axis=0) <= 2).all(), "a bin feeds at most two bands"
    return torch.from_numpy(tab[:FFT].astype(np.float64)), torch.from_numpy(mel)


def _noise(seed, shape, scale=1.0):
    return (scale * np.random.default_rng(seed).uniform(-1.0, 1.0, shape)).astype(np.float32)


def _grad(seed, clips, n_images, n_mels, image_w):
    return np.random.default_rng(2000 + seed).standard_normal((clips, n_images, 1, n_mels, image_w)).astype(np.float32)


def _step(seed, n=4096):
    x = _noise(seed, (1, n), 0.1)
    x[:, n // 2:] *= 1e-5
    return x


def _zerotail(seed, n=4096, cut=2500):
    x = _noise(seed, (1, n), 0.1)
    x[:, cut:] = 0
    return x


def _tonal(n=4096):
    t = np.arange(n, dtype=np.float64)
    return (0.5 * np.sin(2 * np.pi * 1000.0 * t / SR) + 0.05 * np.random.default_rng(15).uniform(-1.0, 1.0, n)).astype(np.float32)[None]


def _dataset_pcm(seed=23):
    """Two 4 s clips of 0.1 noise, the second zero-filled from 60 000 on as the loader fills a short recording. 200 000 - 500 000
    cells of white noise have no unique maximum to speak of (runner-up within 0.003 dB), so each clip also carries one Hann-shaped
    tone burst of 512 samples, centred on a frame of both hops (a multiple of lcm(39, 98) = 3822)."""
    x = _noise(seed, (2, 88200), 0.1)
    x[1, 60000:] = 0
    t = np.arange(-256, 256)
    for clip, (centre, hz) in enumerate(((8 * 3822, 3000.0), (5 * 3822, 1500.0))):
        x[clip, centre - 256:centre + 256] += (0.5 * np.hanning(513)[:512] * np.cos(2 * np.pi * hz * t / SR)).astype(np.float32)
    return x


STEP_SEED, ZEROTAIL_SEED = 1, 6

#           pcm                                  hop  mels images width stride
_SHAPES = {
    "min":      (lambda: _noise(31, (1, 1025)),        98, 224, 1, 11, 0),
    "noise":    (lambda: _noise(32, (2, 4096)),        98, 224, 3, 20, 11),
    "hop39":    (lambda: _noise(33, (1, 4096)),        39, 224, 2, 53, 53),
    "runs":     (lambda: _noise(34, (1, 14000)),       98, 224, 1, 143, 0),
    "mels40":   (lambda: _noise(35, (1, 4096)),        98, 40, 1, 42, 0),
    "step":     (lambda: _step(STEP_SEED),             98, 224, 3, 20, 11),
    "zerotail": (lambda: _zerotail(ZEROTAIL_SEED),     98, 224, 3, 20, 11),
    "tonal":    (_tonal,                               98, 224, 3, 20, 11),
    "silence":  (lambda: np.zeros((1, 4096), np.float32), 98, 224, 3, 20, 11),
    "dataset":  (_dataset_pcm,                         98, 224, 10, 224, 75),
    "dataset39": (_dataset_pcm,                        39, 224, 10, 224, 224),
}
CASES = ("min", "noise", "hop39", "runs", "mels40", "step", "zerotail", "tonal", "floor_only", "silence")     # host simulation and GPU
GPU_ONLY = ("dataset", "dataset39")
FLOOR_CASES = ("step", "zerotail", "floor_only", "dataset", "dataset39")       # cells are clipped: conditioning() must hold
STRIDE_PAD = {"noise": 37}                                                    # the rows of `noise` lie n + 37 elements apart


@functools.lru_cache(maxsize=None)
def case(name, floor_grad=True):
    """Case with read-only tensors: pcm (clips, n) float32, g (clips, images, 1, bands, width) float32."""
    if name == "floor_only":
        base = case("step", floor_grad)
        clipped = split(spectrogram(base.pcm.double(), base, torch.float64)[1], base) < 0
        return base._replace(g=base.g * clipped.float())
    make, hop, n_mels, n_images, image_w, stride = _SHAPES[name]
    pcm = make()
    assert (n_images - 1) * stride + image_w <= frames_of(pcm.shape[1], hop)
    g = _grad(sorted(_SHAPES).index(name), pcm.shape[0], n_images, n_mels, image_w)
    return Case(torch.from_numpy(pcm), torch.from_numpy(g), hop, n_mels, n_images, image_w, stride, floor_grad)


def split(d, c):
    """(clips, bands, frames) -> (clips, images, 1, bands, width)"""
    return torch.stack([d[:, :, t * c.stride:t * c.stride + c.image_w] for t in range(c.n_images)], dim=1)[:, :, None]


def spectrogram(x, c, dtype):
    """x (clips, n) of `dtype` -> (D (clips, bands, frames) before the floor, D - floor (the same shape)); differentiable."""
    win, mel = (t.to(dtype) for t in tables(c.n_mels))
    p = torch.nn.functional.pad(x[:, None], (PAD, PAD), mode="reflect")[:, 0]
    spec = torch.fft.rfft(p.unfold(-1, FFT, c.hop) * win)
    power = spec.real * spec.real + spec.imag * spec.imag
    d = (10.0 * torch.log10(torch.clamp(power @ mel.T, min=AMIN))).transpose(1, 2)
    floor = d.reshape(d.shape[0], -1).max(dim=1).values - TOP_DB
    return d, d - floor[:, None, None]


def images_of(d, c):
    """maximum(D, D.max() - top_db) and the split; with floor_grad False the floor is a constant."""
    floor = d.reshape(d.shape[0], -1).max(dim=1).values - TOP_DB
    if not c.floor_grad:
        floor = floor.detach()
    return split(torch.maximum(d, floor[:, None, None]), c)


def autograd_grads(c, dtype):
    """(d L / d D (clips, bands, frames), d L / d pcm (clips, n)) for L = sum(images * G), by torch.autograd in `dtype`."""
    x = c.pcm.to(dtype).clone().requires_grad_(True)
    d, _ = spectrogram(x, c, dtype)
    d.retain_grad()
    (images_of(d, c) * c.g.to(dtype)).sum().backward()
    return d.grad.detach(), x.grad.detach()


@functools.lru_cache(maxsize=None)
def reference(name, floor_grad=True):
    """float64 (d_db, d_pcm)."""
    return autograd_grads(case(name, floor_grad), torch.float64)


@functools.lru_cache(maxsize=None)
def restatement(name, floor_grad=True):
    """float32 (d_db, d_pcm) by torch on the CPU: not the code under test."""
    return autograd_grads(case(name, floor_grad), torch.float32)


def err(got, ref):
    scale = float(ref.abs().max())
    diff = float((got.double() - ref).abs().max())
    return diff / scale if scale > 0 else diff


def yardstick(name, which, floor_grad=True):
    """err of the float32 restatement on the case; which: 0 = d_db, 1 = d_pcm."""
    return err(restatement(name, floor_grad)[which], reference(name, floor_grad)[which])


def bound(name, which, floor_grad=True):
    return YARDSTICK_FACTOR * yardstick(name, which, floor_grad)


@functools.lru_cache(maxsize=None)
def conditioning(name):
    """(gap of the maximum to the runner-up in dB, least distance of a cell to the floor in dB, the float32 restatement's largest
    dB error over the cells within NEAR_DB of the floor -- 0.0 where there is none), the worst clip of the case, in float64."""
    c = case(name)
    with torch.no_grad():
        d64, rel64 = spectrogram(c.pcm.double(), c, torch.float64)
        d32, _ = spectrogram(c.pcm.float(), c, torch.float32)
    top = d64.reshape(d64.shape[0], -1).topk(2, dim=1).values
    gap = float((top[:, 0] - top[:, 1]).min())
    margin = float(rel64.abs().min())
    near = rel64.abs() <= NEAR_DB
    near_err = float((d32.double() - d64)[near].abs().max()) if bool(near.any()) else 0.0
    return gap, margin, near_err


def loop_form(c):
    """The formulas of DESIGN.md 3.17, clip by clip and frame by frame in float64 with explicit cos / sin sums -> (d_db, d_pcm)."""
    win, mel = tables(c.n_mels)
    x = c.pcm.double()
    clips, n = x.shape
    frames = frames_of(n, c.hop)
    k, m = torch.arange(BINS, dtype=torch.float64), torch.arange(FFT, dtype=torch.float64)
    ang = 2 * np.pi / FFT * torch.outer(k, m)
    cos, sin = torch.cos(ang), torch.sin(ang)
    g = c.g.double()
    d_db, d_pcm = torch.zeros(clips, c.n_mels, frames, dtype=torch.float64), torch.zeros_like(x)
    for ci in range(clips):
        y = x[ci]
        refl = lambda j: -j if j < 0 else 2 * (n - 1) - j if j >= n else j                       # noqa: E731
        p = torch.stack([y[refl(q - PAD)] for q in range(n + 2 * PAD)])
        xs, S = [], torch.zeros(c.n_mels, frames, dtype=torch.float64)
        for f in range(frames):
            xf = win * p[f * c.hop:f * c.hop + FFT]
            xr, xi = cos @ xf, -(sin @ xf)
            xs.append((xr, xi))
            S[:, f] = mel @ (xr * xr + xi * xi)
        D = 10.0 * torch.log10(torch.clamp(S, min=AMIN))
        floor = D.max() - TOP_DB
        gD = torch.zeros_like(D)
        for t in range(c.n_images):
            gD[:, t * c.stride:t * c.stride + c.image_w] += g[ci, t, 0]
        dD = torch.where(D > floor, gD, torch.zeros_like(gD))
        if c.floor_grad:
            flat = int(torch.argmax((D == D.max()).flatten().to(torch.int8)))                    # the first cell that holds the maximum
            dD[flat // frames, flat % frames] += gD[D < floor].sum()
        d_db[ci] = dD
        dp = torch.zeros(n + 2 * PAD, dtype=torch.float64)
        for f in range(frames):
            xr, xi = xs[f]
            r = torch.where(S[:, f] > AMIN, dD[:, f] * (10.0 / np.log(10.0)) / torch.clamp(S[:, f], min=AMIN), torch.zeros(c.n_mels, dtype=torch.float64))
            dP = mel.T @ r
            ur, ui = 2 * dP * xr, 2 * dP * xi
            dp[f * c.hop:f * c.hop + FFT] += win * (ur @ cos - ui @ sin)
        for s in range(n):
            v = dp[PAD + s]
            if 1 <= s <= PAD:
                v = v + dp[PAD - s]
            if n - 1 - PAD <= s <= n - 2:
                v = v + dp[PAD + 2 * (n - 1) - s]
            d_pcm[ci, s] = v
    return d_db, d_pcm
