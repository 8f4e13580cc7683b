"""Cases, operands, float64 references, bounds and numpy restatements of tests/test_dropin_kernels_gpu.py, callable without a device
(tests/test_dropin_kernel_cases_cpu.py evaluates every case, every exactness claim and every share condition on the CPU).

Six stand-alone kernels of csrc/stft_generic.hip: stft_kernel, mel_log_kernel, dataset_frames_kernel, postprocess_kernel,
mono_mix_kernel and resample_kernel. Nothing here is an oracle for VALUES except numpy float64 arithmetic on the stored operands
(and oracle/resample.py, the float64 statement of the resampler). The constants the shapes depend on are read from the source with
_one(), so a rewritten definition fails the regular expression instead of silently untesting a branch.

Criteria, as in tests/pin_leftover_cases.py:
  exact     operands on a dyadic grid; the case asserts sum|terms| / unit < 2^24 from its own float64 reference, so every partial sum
            in any order is an f32 value; gathers and double-precision means rounded once are bit-equal by construction;
  derived   |got - ref| <= P 2^-24 sum|terms| per element, P counted in the docstring of the bound;
  yardstick the broadband STFT figure: the same figure of fft_f32(), a plain f32 restatement of the kernel's transform;
  measured  logf alone (tests/test_dropin_kernels_gpu.py, table MEASURED)."""

import functools
import importlib
import re
from fractions import Fraction

import numpy as np

from conftest import PKG
from infer_kernel_cases import U, _one, _source
from oracle import resample as ors

mel_features = importlib.import_module(PKG + ".torchvggish.mel_features")

F32 = np.float32


# ------------------------------------------------------------------------------------------------ constants ----

def _constants():
    src = _source("csrc/stft_generic.hip")
    c = {"max_fft": int(_one(r"constexpr int kMaxFft = (\d+);", src, "kMaxFft"))}
    # stft_kernel: 256 lanes stride over the fft points, the fft / 2 butterflies of a stage and the bins
    assert len(re.findall(r"for \(int \w+ = threadIdx\.x; \w+ < (?:fft|fft / 2|bins); \w+ \+= 256\)", src)) == 3, "stft_kernel's lane loops"
    _one(r"hipLaunchKernelGGL\(stft_kernel, dim3\(unsigned\(frames\)\), dim3\(256\), size_t\(2 \* fft_length \* sizeof\(float\)\),", src, "stft_kernel's launch")
    c["stft_lanes"] = 256
    # mel_log_kernel: one lane per output, 256 per block
    _one(r"const int64_t i = int64_t\(blockIdx\.x\) \* 256 \+ threadIdx\.x;\n    if \(i >= frames \* bands\) return;", src, "mel_log_kernel's index")
    _one(r"hipLaunchKernelGGL\(mel_log_kernel, dim3\(unsigned\(\(frames \* bands \+ 255\) / 256\)\), dim3\(256\),", src, "mel_log_kernel's launch")
    c["mel_lanes"] = 256
    # dataset_frames_kernel: grid-stride over the outputs, at most 8192 blocks of 256 lanes
    _one(r"for \(int64_t i = int64_t\(blockIdx\.x\) \* 256 \+ threadIdx\.x; i < total; i \+= int64_t\(gridDim\.x\) \* 256\) \{", src, "dataset_frames_kernel's loop")
    cap = _one(r"hipLaunchKernelGGL\(dataset_frames_kernel, dim3\(unsigned\(\(total \+ 255\) / 256 < (\d+) \? \(total \+ 255\) / 256 : (\d+)\)\), dim3\(256\),", src,
               "dataset_frames_kernel's grid cap")
    assert cap[0] == cap[1]
    c["frames_blocks"], c["frames_lanes"] = int(cap[0]), 256
    c["frames_columns"] = int(_one(r"MLA_REQUIRE\(\(int64_t\(n_frames\) - 1\) \* stride \+ frame_len <= (\d+), MLA_E_SHAPE,", src, "the spectrogram's width"))
    c["frames_slots"] = int(_one(r"ex_per_clip >= 0 && ex_per_clip <= (\d+) &&", src, "the slots of a clip"))
    # postprocess_kernel: one block of 128 lanes per row; mono_mix / resample: one lane per output, 256 per block
    _one(r"hipLaunchKernelGGL\(postprocess_kernel, dim3\(unsigned\(rows\)\), dim3\(128\),", src, "postprocess_kernel's launch")
    _one(r"const unsigned grid = unsigned\(\(n_samples \+ 255\) / 256\);", src, "mono_mix_kernel's grid")
    _one(r"hipLaunchKernelGGL\(resample_kernel, dim3\(unsigned\(\(n_out \+ 255\) / 256\)\), dim3\(256\),", src, "resample_kernel's launch")
    return c


C = _constants()


# -------------------------------------------------------------------------------------------- 1. stft_kernel ----

def _sweep(p):
    fft = 1 << p
    win = max(1, 3 * fft // 4 - 1)
    return fft, win, max(1, win // 3)


# (fft, win, hop): every power of two up to kMaxFft with a window below it, then the named ones; hop > win at (64, 10, 37)
STFT_CONFIGS = tuple(dict.fromkeys(
    [_sweep(p) for p in range(1, C["max_fft"].bit_length())]
    + [(2, 2, 1), (2, 1, 1), (4, 3, 2), (8, 8, 3), (256, 200, 80), (512, 400, 160), (1024, 1000, 999), (4096, 4096, 4096), (4096, 2500, 1000),
       (64, 10, 37)]))
STFT_KINDS = ("noise", "impulses", "constant", "cosine")
STFT_R_MAX = 5e-7                                # the condition on the restatement's own broadband figure


def stft_id(cfg):
    return "fft%d-win%d-hop%d" % cfg


def stft_frames(n, win, hop):
    return 1 + (n - win) // hop if n >= win else 0


def stft_lengths(cfg):
    """n == win (one frame), win + hop - 1 (still one), win + hop (two), and a length of 3, 4 or 5 frames that ends inside a hop."""
    fft, win, hop = cfg
    many = 3 + (fft.bit_length() + win) % 3
    return (win, win + hop - 1, win + hop, win + (many - 1) * hop + (hop - 1) // 2)


def stft_p(fft):
    """f32 roundings of one output against S = sum_n |x_n w_n| of its frame, counted in stft_kernel whichever way the compiler
    contracts multiply-adds. Every value the transform holds is a sum of the frame's products under unit-modulus factors: at most S.
       1  x[n] * window[n];
    per stage, log2(fft) of them, on the complex value z:
       1  the twiddle: (cos, -sin) rounded from double, each component within 2^-25, the pair within 2^-24;
       3  t = z w: per component two products and one subtraction; |re wr| + |im wi| <= |z|, so the products cost 2^-24 |z| per
          component and the subtraction 2^-24 |t_c|: sqrt(2) + 1 < 3 for the pair;
       1  u +- t: one rounding per component, 2^-24 |result| for the pair;
    magnitude sqrtf(re re + im im):
       3  two squares and their sum are 2 roundings of re^2 + im^2, which the square root halves; the root's own rounding;
          one spare for what the complex error does to |.| at second order.
    P = 5 log2(fft) + 4."""
    return 5 * (fft.bit_length() - 1) + 4


def stft_window(win):
    """The f32 Hann window frontend.stft_magnitude uploads."""
    return mel_features.periodic_hann(win).astype(F32)


def stft_twiddle(fft):
    """The f32 (cos, -sin)(2 pi m / fft), m < fft / 2, frontend.stft_magnitude uploads."""
    m = np.arange(fft // 2)
    return np.stack([np.cos(2 * np.pi * m / fft), -np.sin(2 * np.pi * m / fft)], axis=1).astype(F32)


def stft_signal(cfg, n, kind):
    """The f32 input of a case. noise: uniform in [-1, 1). impulses: zeros with 1.0 and -0.75 planted in every frame; frame 0 has
    its 1.0 at sample 0 and the last frame at sample win - 1. constant: 0.625. cosine: on bin fft / 4, cos(pi n / 2)."""
    fft, win, hop = cfg
    rng = np.random.default_rng([fft, win, hop, n, STFT_KINDS.index(kind)])
    if kind == "noise":
        return (rng.random(n) * 2 - 1).astype(F32)
    if kind == "constant":
        return np.full(n, 0.625, dtype=F32)
    if kind == "cosine":
        return np.cos(2 * np.pi * (fft / 4) * np.arange(n) / fft).astype(F32)
    x = np.zeros(n, dtype=F32)
    frames = stft_frames(n, win, hop)
    for f in range(frames):
        x[f * hop + int(rng.integers(0, win))] = -0.75
    for f in range(frames):
        x[f * hop + (0 if f == 0 else win - 1 if f == frames - 1 else int(rng.integers(0, win)))] = 1.0
    if frames == 1 and win > 1:                                     # one frame: both ends
        x[win - 1] = -0.75
    return x


def stft_products64(cfg, x):
    """(frames, win) float64 products of the stored operands: float32(x) and the f32 window."""
    fft, win, hop = cfg
    frames = stft_frames(x.shape[0], win, hop)
    idx = np.arange(frames)[:, None] * hop + np.arange(win)[None, :]
    return x.astype(np.float64)[idx] * stft_window(win).astype(np.float64)[None, :]


def stft_reference(cfg, x):
    """abs(np.fft.rfft(frames64 * win32, fft)) in float64 and S = sum_n |x_n w_n| per frame."""
    prod = stft_products64(cfg, x)
    return np.abs(np.fft.rfft(prod, cfg[0], axis=1)), np.abs(prod).sum(axis=1)


def fft_f32(cfg, x):
    """stft_kernel restated in numpy f32, operation by operation and with NO contraction: the window product, the bit-reversed
    load, log2(fft) radix-2 decimation-in-time stages with the same f32 twiddles, sqrt(re re + im im). (frames, fft / 2 + 1) f32."""
    fft, win, hop = cfg
    lg = fft.bit_length() - 1
    frames = stft_frames(x.shape[0], win, hop)
    idx = np.arange(frames)[:, None] * hop + np.arange(win)[None, :]
    v = np.zeros((frames, fft), dtype=F32)
    v[:, :win] = x[idx] * stft_window(win)[None, :]
    rev = np.array([int(format(i, "0%db" % lg)[::-1], 2) for i in range(fft)])
    re, im = np.zeros_like(v), np.zeros_like(v)
    re[:, rev] = v
    tw = stft_twiddle(fft)
    b = np.arange(fft // 2)
    for s in range(1, lg + 1):
        half, step = 1 << (s - 1), fft >> s
        grp, pos = b // half, b % half
        i0 = grp * 2 * half + pos
        i1 = i0 + half
        wr, wi = tw[pos * step, 0][None, :], tw[pos * step, 1][None, :]
        tr = re[:, i1] * wr - im[:, i1] * wi
        ti = re[:, i1] * wi + im[:, i1] * wr
        ur, ui = re[:, i0].copy(), im[:, i0].copy()
        re[:, i0], im[:, i0] = ur + tr, ui + ti
        re[:, i1], im[:, i1] = ur - tr, ui - ti
    k = fft // 2 + 1
    out = np.sqrt(re[:, :k] * re[:, :k] + im[:, :k] * im[:, :k])
    assert out.dtype == F32
    return out


def stft_frame_errors(got, ref):
    """Per frame ||got - ref||_2 / ||ref||_2 in float64; a frame whose reference is all zero gives 0 when got is, inf otherwise."""
    d = np.sqrt(((got.astype(np.float64) - ref) ** 2).sum(axis=1))
    r = np.sqrt((ref ** 2).sum(axis=1))
    return np.where(r > 0, d / np.where(r > 0, r, 1.0), np.where(d > 0, np.inf, 0.0))


def stft_worst_ratio(got, ref, s, fft):
    """max |got - ref| / (P 2^-24 S) over the elements; an element whose bound is 0 must be equal (ratio 0, or inf)."""
    bound = stft_p(fft) * U * s[:, None]
    err = np.abs(got.astype(np.float64) - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


@functools.lru_cache(maxsize=None)
def stft_case(cfg):
    """Per length and kind: the signal, the float64 reference and S; and R of the configuration -- the largest per-frame broadband
    figure of fft_f32() over the noise signals of all its lengths."""
    items, r = {}, 0.0
    for n in stft_lengths(cfg):
        for kind in STFT_KINDS:
            x = stft_signal(cfg, n, kind)
            ref, s = stft_reference(cfg, x)
            items[(n, kind)] = dict(x=x, ref=ref, s=s)
            if kind == "noise":
                e = stft_frame_errors(fft_f32(cfg, x), ref)
                assert np.isfinite(e).all()
                r = max(r, float(e.max()))
    return dict(items=items, R=r)


# ----------------------------------------------------------------------------------------- 2. mel_log_kernel ----

MEL_SHAPES = ((1, 2, 1), (3, 129, 20), (13, 257, 64), (5, 257, 65), (2, 2049, 128), (1, 33, 300))      # (frames, bins, bands)
MEL_OFFSETS = (0.0, 2.0 ** -6, 1.0)
MEL_MIN_LOG = 2.0 ** -6                          # |log v| of every finite result but the planted exact 0
LOGF_CAP = 4 * U                                 # the measured logf bound never exceeds this relative error


def mel_id(shape):
    return "%dx%dx%d" % shape


@functools.lru_cache(maxsize=None)
def mel_grid_case(shape, offset):
    """spec: multiples of 2^-3 in [0, 4], mel: multiples of 2^-3 in [0, 1]; every product is a multiple of 2^-6 and the sum of a
    column is asserted below 2^24 of them, so acc is an f32 value in any order and v = acc + offset is known exactly (offsets 0,
    2^-6, 1 are on the grid). Planted where the shape has room: a silent last frame (frames >= 2) and an all-zero last mel column
    (bands >= 3) -- at offset 0 they give v = 0, at offset 1 v = 1 --, and a one-hot column bands - 2 whose single weight, on the
    last bin, meets spec[0] such that v == 1 exactly (1 . 1 at offset 0, 9/8 . 7/8 + 2^-6). No other v equals 65/64, the one grid
    value with 0 < |log v| < 2^-6: a draw that has one is drawn again."""
    frames, bins, bands = shape
    for attempt in range(100):
        rng = np.random.default_rng([frames, bins, bands, int(offset * 64), attempt])
        spec = (rng.integers(0, 33, (frames, bins)) / 8.0).astype(F32)
        mel = (rng.integers(0, 9, (bins, bands)) / 8.0).astype(F32)
        one = None
        if frames >= 2:
            spec[frames - 1] = 0.0
        if bands >= 3:
            mel[:, bands - 1] = 0.0
            mel[:, bands - 2] = 0.0
            sa, mb = {0.0: (8, 8), 2.0 ** -6: (9, 7), 1.0: (0, 8)}[offset]
            mel[bins - 1, bands - 2], spec[0, bins - 1] = mb / 8.0, sa / 8.0
            one = (0, bands - 2)
        elif offset == 1.0:
            spec[0] = 0.0
            one = (0, 0)
        else:                                    # (1, 2, 1): the only column is the one-hot one
            sa, mb = (8, 8) if offset == 0.0 else (9, 7)
            mel[:, 0] = 0.0
            mel[bins - 1, 0], spec[0, bins - 1] = mb / 8.0, sa / 8.0
            one = (0, 0)
        s64, m64 = spec.astype(np.float64), mel.astype(np.float64)
        acc = s64 @ m64
        assert float((np.abs(s64) @ np.abs(m64)).max()) / 2.0 ** -6 < 2.0 ** 24
        v = acc + offset
        assert np.array_equal(v, v.astype(F32).astype(np.float64)) and np.array_equal(v * 64, np.rint(v * 64))
        with np.errstate(divide="ignore"):
            ref = np.log(v)
        finite = np.isfinite(ref)
        if bool(((np.abs(ref) < MEL_MIN_LOG) & finite & (v != 1.0)).any()):
            continue
        assert v[one] == 1.0
        return dict(spec=spec, mel=mel, v=v, ref=ref, one=one)
    raise AssertionError("no draw without a value next to 1")


def mel_f32_chain(spec, mel, offset):
    """v of mel_log_kernel in numpy f32: products and sums rounded one by one, k ascending, then the offset (no contraction)."""
    acc = np.zeros((spec.shape[0], mel.shape[1]), dtype=F32)
    for k in range(spec.shape[1]):
        acc = acc + spec[:, k:k + 1] * mel[k:k + 1, :]
    out = acc + F32(offset)
    assert out.dtype == F32
    return out


MEL_UNIFORM = {  # id -> (frames, bins, mel matrix arguments, offset)
    "16k-0.01": (13, 257, dict(num_mel_bins=64, num_spectrogram_bins=257, audio_sample_rate=16000, lower_edge_hertz=125.0, upper_edge_hertz=7500.0), 0.01),
    "16k-0": (13, 257, dict(num_mel_bins=64, num_spectrogram_bins=257, audio_sample_rate=16000, lower_edge_hertz=125.0, upper_edge_hertz=7500.0), 0.0),
    "8k-0.01": (3, 129, dict(), 0.01),
    "8k-0": (3, 129, dict(), 0.0),
}


@functools.lru_cache(maxsize=None)
def mel_uniform_case(cid):
    """spec uniform in [0, 30), the real matrix of spectrogram_to_mel_matrix rounded to f32 as frontend.log_mel_spectrogram uploads
    it. acc is a chain of `bins` fused multiply-adds from +0 and one addition of the offset: (bins + 1) roundings against
    sum|terms| (= acc here: no term is negative); in the log domain that is (bins + 1) 2^-24 sum|terms| / (acc + offset) (to first
    order: the quotient is below 2e-5), to which the test adds the logf term."""
    frames, bins, kw, offset = MEL_UNIFORM[cid]
    rng = np.random.default_rng([frames, bins, int(offset * 100)])
    spec = (rng.random((frames, bins)) * 30).astype(F32)
    mel = mel_features.spectrogram_to_mel_matrix(**kw).astype(F32)
    assert mel.shape[0] == bins
    off32 = float(F32(offset))                   # the offset travels as a C float
    acc = spec.astype(np.float64) @ mel.astype(np.float64)
    terms = np.abs(spec.astype(np.float64)) @ np.abs(mel.astype(np.float64))
    v = acc + off32
    with np.errstate(divide="ignore"):
        ref = np.log(v)
    bound = (bins + 1) * U * terms / np.where(v > 0, v, 1.0)
    return dict(spec=spec, mel=mel, offset=off32, ref=ref, bound=bound)


# ---------------------------------------------------------------------------------- 3. dataset_frames_kernel ----

FRAMES_GEOMETRIES = ((10, 96, 32), (4, 96, 96), (1, 384, 0), (1, 1, 0), (289, 96, 1), (5, 7, 13), (3, 96, 0))      # (n_frames, frame_len, stride)
FRAMES_SLOTS = (0, 1, 2, 3, 4)
FRAMES_CLIPS = (1, 3, 35)                         # at (10, 96, 32); the other geometries run 3 clips, (289, 96, 1) one (7 MB)
FRAMES_BIG = (35, 4, (10, 96, 32))


def frames_cases():
    """(clips, ex_per_clip, geometry): every geometry with every slot count at 3 clips (289 frames: 1); 1 and 35 clips at (10, 96, 32)."""
    out = [(1 if g[0] == 289 else 3, e, g) for g in FRAMES_GEOMETRIES for e in FRAMES_SLOTS]
    out += [(1, 4, FRAMES_GEOMETRIES[0]), (1, 1, FRAMES_GEOMETRIES[0]), FRAMES_BIG, (35, 3, FRAMES_GEOMETRIES[0])]
    return out


def frames_id(case):
    return "clips%d-ex%d-%dx%d+%d" % ((case[0], case[1]) + case[2])


def frames_examples(clips, ex_per_clip):
    """(clips * ex_per_clip, 96, 64) f32 holding 1, 2, 3, ...: distinct, never the 0.0 of a missing slot, exact up to 2^24."""
    n = clips * ex_per_clip * 96 * 64
    assert n < 2 ** 24
    return (np.arange(n, dtype=np.float64) + 1).astype(F32).reshape(clips * ex_per_clip, 96, 64)


def frames_restated(ex, clips, ex_per_clip, geometry):
    """The index rule of dataset.py:318-363 as csrc/stft_generic.hip states it: spec_c[band][slot * 96 + fr] = ex[c][slot][fr][band]
    for slot < ex_per_clip and 0.0 in the slots a clip lacks (384 columns); out[c][t][band][x] = spec_c[band][t * stride + x]."""
    n_frames, frame_len, stride = geometry
    spec = np.zeros((clips, 64, C["frames_columns"]), dtype=F32)
    if ex_per_clip:
        e = ex.reshape(clips, ex_per_clip, 96, 64)
        spec[:, :, :96 * ex_per_clip] = e.transpose(0, 3, 1, 2).reshape(clips, 64, 96 * ex_per_clip)
    out = np.zeros((clips, n_frames, 64, frame_len), dtype=F32)
    for t in range(n_frames):
        out[:, t] = spec[:, :, t * stride:t * stride + frame_len]
    return out


def frames_trips(clips, geometry):
    """(outputs, lanes of one trip through the capped grid)."""
    n_frames, frame_len, _ = geometry
    return clips * n_frames * 64 * frame_len, C["frames_blocks"] * C["frames_lanes"]


# ------------------------------------------------------------------------------------- 4. postprocess_kernel ----

POST_ROWS = (1, 3, 1000)
POST_P = 130


@functools.lru_cache(maxsize=None)
def post_grid_case():
    """E: integers -8..8 over 64; mu: multiples of 2^-4 in [-1, 1]; x = mu + d with d multiples of 2^-4 in [-2, 2]. x - mu is exact,
    every product is a multiple of 2^-10, |acc| <= 128 . (1/8) . 2 = 32 = 2^15 units; clamp(acc) + 2 <= 4 is at most 12 bits of
    2^-10 and times 63.75 = 255 / 4 (8 bits) a multiple of 2^-12 below 2^8: 20 bits. Every step is an f32 value, so the kernel's
    result must be rint of the float64 value. (A dyadic acc ties only at acc == 0, where 127.5 -> 128 under round-half-even AND
    round-half-up: this grid cannot tell the two rules apart and does not claim to.)
    Rows of the 1000-row case: 0: x == mu (all 128); 1: d = 2 on k < 9 and 2: d = 2 on k < 8, -2 at k = 8, against the planted rows
    5..8 of E (+-1/8 on k < 8 resp. k < 9, zero elsewhere): acc exactly +2, -2, +2.25, -2.25 in row 1; 3..130: one-hot d = +-2 at
    k = row - 3, which reads E column by column; the rest random. The 3-row case is rows 0..2, the 1-row case row 500."""
    rng = np.random.default_rng(4242)
    E = rng.integers(-8, 9, (128, 128)) / 64.0
    E[5:9] = 0.0
    E[5, :8], E[6, :8], E[7, :9], E[8, :9] = 0.125, -0.125, 0.125, -0.125
    mu = rng.integers(-16, 17, 128) / 16.0
    d = rng.integers(-32, 33, (1000, 128)) / 16.0
    d[0] = 0.0
    d[1], d[2] = 0.0, 0.0
    d[1, :9] = 2.0
    d[2, :8], d[2, 8] = 2.0, -2.0
    d[3:131] = 0.0
    d[np.arange(3, 131), np.arange(128)] = np.where(np.arange(128) % 2 == 0, 2.0, -2.0)
    x = mu[None, :] + d
    E32, mu32, x32 = E.astype(F32), mu.astype(F32), x.astype(F32)
    assert np.array_equal(E32, E) and np.array_equal(mu32, mu) and np.array_equal(x32, x)
    ref = post_reference(x32, E32, mu32)
    return dict(E=E32, mu=mu32, x=x32, **ref)


def post_reference(x, E, mu):
    """float64 on the stored operands: acc[n][j] = sum_k E[j][k] (x[n][k] - mu[k]), v = (clamp(acc, -2, 2) + 2) 63.75, and
    sum|terms| per output."""
    d = x.astype(np.float64) - mu.astype(np.float64)[None, :]
    acc = d @ E.astype(np.float64).T
    terms = np.abs(d) @ np.abs(E.astype(np.float64)).T
    v = (np.clip(acc, -2.0, 2.0) + 2.0) * 63.75
    return dict(acc=acc, terms=terms, v=v, q=np.rint(v))


def post_rows(case, rows):
    return case["x"][500:501] if rows == 1 else case["x"][:rows]


def post_f32_emulation(x, E, mu):
    """The kernel's chain in numpy f32 (products and sums rounded one by one, k ascending): on the grid every step is exact."""
    d = x - mu[None, :]
    acc = np.zeros((x.shape[0], 128), dtype=F32)
    for k in range(128):
        acc = acc + d[:, k:k + 1] * E[None, :, k]
    acc = np.minimum(np.maximum(acc, F32(-2.0)), F32(2.0))
    out = np.rint((acc + F32(2.0)) * (F32(255.0) / F32(4.0)))
    assert out.dtype == F32
    return out


@functools.lru_cache(maxsize=None)
def post_uniform_case():
    """x uniform in [0, 2), mu in [0, 1), E uniform in [-0.15, 0.15): acc has a standard deviation near 0.8, so most outputs stay
    interior. 300 rows. tie[n][j] = |frac(v) - 0.5|, the distance of the float64 value to the nearest rounding tie, and the derived
    bound 63.75 . 130 . 2^-24 . sum|terms| in the same units (one rounding of x - mu, 128 of the chain, the +2 -- the product with
    63.75 is the last): where tie > bound the result is rint(v), elsewhere either neighbour."""
    rng = np.random.default_rng(4343)
    E = ((rng.random((128, 128)) * 2 - 1) * 0.15).astype(F32)
    mu = rng.random(128).astype(F32)
    x = (rng.random((300, 128)) * 2).astype(F32)
    ref = post_reference(x, E, mu)
    tie = np.abs(ref["v"] - np.floor(ref["v"]) - 0.5)
    return dict(E=E, mu=mu, x=x, tie=tie, bound=63.75 * POST_P * U * ref["terms"], **ref)


def post_uniform_ok(got, c):
    """Elementwise: got == rint(v) where the tie is farther than the bound, else got is floor(v) or ceil(v)."""
    got = got.astype(np.float64)
    sure = c["tie"] > c["bound"]
    return np.where(sure, got == c["q"], (got == np.floor(c["v"])) | (got == np.ceil(c["v"])))


# --------------------------------------------------------------------------------------- 5. mono_mix_kernel ----

MIX_CHANNELS = (2, 3, 5, 8)
MIX_NS = (1, 255, 256, 257, 70001)


def mix_input(n, channels, pcm16):
    """(n, channels) int16 over the whole range with frames of all -32768, all 32767 and the two alternating planted in front
    (as many as fit), or float32 uniform in [-1, 1)."""
    rng = np.random.default_rng([n, channels, int(pcm16)])
    if not pcm16:
        return (rng.random((n, channels)) * 2 - 1).astype(F32)
    a = rng.integers(-32768, 32768, (n, channels)).astype(np.int16)
    planted = np.array([[-32768] * channels, [32767] * channels, [(-32768, 32767)[c % 2] for c in range(channels)]], dtype=np.int16)
    if n == 1:
        a[0] = planted[2]
    else:
        a[:min(n, 3)] = planted[:min(n, 3)]
    return a


def mix_reference(a):
    """resample_core.h's mono_mix_as in float64: the channels added one by one, divided by their count, times 2^-15 for int16
    (1 for float32), cast once to f32."""
    acc = np.zeros(a.shape[0], dtype=np.float64)
    for c in range(a.shape[1]):
        acc = acc + a[:, c].astype(np.float64)
    scale = 1.0 / 32768.0 if a.dtype == np.int16 else 1.0
    return (acc / float(a.shape[1]) * scale).astype(F32)


# ---------------------------------------------------------------------------------------- 6. resample_kernel ----

RESAMPLE_CASES = ((44100, 3000), (22050, 2500), (48000, 3001), (8000, 900), (11025, 1200), (256000, 9000), (44100, 3), (48000, 63))     # (sr, n) -> 16 kHz
RESAMPLE_SHORT = (44100, 1)                      # int(1 . 16000 / 44100) = 0 outputs: ValueError on both sides
RESAMPLE_KINDS = ("noise", "impulse-first", "impulse-last")
SR_OUT = 16000
RESAMPLE_DOUBLE = 1e-10                          # times max|x|: the kernel's fma position against the oracle's t * (1 / ratio)


def resample_id(case):
    return "%d-n%d" % case


def resample_signal(case, kind):
    sr, n = case
    if kind == "noise":
        return (np.random.default_rng([sr, n]).random(n) * 2 - 1).astype(F32)
    x = np.zeros(n, dtype=F32)
    x[0 if kind == "impulse-first" else n - 1] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def resample_case(case, kind):
    """The signal, oracle/resample.py on its f32-rounded values, and the bound 2^-24 |ref| + 1e-10 max|x|: the one f32 rounding of
    the double accumulator, and the double-precision difference between the two statements of the position."""
    x = resample_signal(case, kind)
    ref = ors.resample(x.astype(np.float64), case[0], SR_OUT)
    return dict(x=x, ref=ref, bound=U * np.abs(ref) + RESAMPLE_DOUBLE * float(np.abs(x).max()))


def resample_geometry(case):
    """(outputs, table step, most taps of a wing) at the 'kaiser_best' table (512 entries per crossing, 64 crossings)."""
    sr, n = case
    ratio = float(SR_OUT) / float(sr)
    step = int(min(1.0, ratio) * 512)
    return int(n * ratio), step, (64 * 512 + 1) // step


def resample_restated(x, sr):
    """resample_core.h's setup() and wings() in numpy float64 for every output at once: the position's fractional part by ONE
    rounding of inv * t - n (an exact fused multiply-add, taken from rationals), the table read by win + eta * delta, left wing
    first. The inner fused multiply-adds are written as plain double operations: 2^-53 relative per tap."""
    x = x.astype(np.float64)
    ratio = float(SR_OUT) / float(sr)
    n_in, n_out = x.shape[0], int(x.shape[0] * ratio)
    win, num_table = ors.sinc_window()
    scale = min(1.0, ratio)
    win = win * ratio if ratio < 1 else win
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    step, nwin, inv = int(scale * num_table), win.shape[0], 1.0 / ratio
    t = np.arange(n_out, dtype=np.float64)
    n = (t * inv).astype(np.int64)
    frac_l = scale * np.array([float(Fraction(inv) * int(tt) - int(nn)) for tt, nn in zip(t, n)])
    y = np.zeros(n_out)
    for frac, sign in ((frac_l, -1), (scale - frac_l, 1)):
        idx_f = frac * float(num_table)
        off = idx_f.astype(np.int64)
        eta = idx_f - off
        most = np.minimum(n + 1 if sign < 0 else n_in - n - 1, (nwin - off) // step)
        for i in range(int(most.max()) if most.size else 0):
            m = i < most
            idx = off[m] + i * step
            y[m] += (win[idx] + eta[m] * delta[idx]) * x[n[m] - i if sign < 0 else n[m] + i + 1]
    return y
