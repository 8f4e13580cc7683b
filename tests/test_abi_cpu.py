"""CPU tests of the C-ABI library and of the kernel arithmetic simulated on the host.

No compute entry point is called here (no GPU in this container): the library must load,
export every symbol include/mla_hip.h declares, and its host-side helpers (frame counts,
constant tables) must agree with the oracle. The per-lane kernel math (csrc/logmel_core.h)
is compiled with g++ and run lane by lane against the oracle.
"""

import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from oracle import frontend as ofe


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


def test_library_exports_every_declared_symbol(L):
    lib = L.lib()
    names = L.declared_symbols()
    assert "mla_logmel_examples" in names and len(names) >= 7
    for n in names:
        assert hasattr(lib, n), n
    assert lib.mla_abi_version() >= 1


def test_counts_match_reference_table(L, golden):
    lib = L.lib()
    f, e = ctypes.c_int64(), ctypes.c_int64()
    for n, n_ex, raised in golden("frontend")["count_table"]:
        rc = lib.mla_logmel_counts(int(n), ctypes.byref(f), ctypes.byref(e))
        if raised:
            assert rc == L.E_SHORT and b"ValueError" in lib.mla_last_error()
        else:
            assert rc == 0 and e.value == n_ex and f.value == ofe.num_frames(int(n), 400, 160)
    for n in range(0, 40000, 37):
        rc = lib.mla_logmel_counts(n, ctypes.byref(f), ctypes.byref(e))
        if n < 240:
            assert rc == L.E_SHORT
        else:
            assert rc == 0 and (f.value, e.value) == (ofe.num_frames(n, 400, 160), ofe.num_examples(n))


def test_tables_match_oracle(L):
    lib = L.lib()
    win, mel = np.zeros(400), np.zeros((257, 64))
    assert lib.mla_logmel_reference_tables(win.ctypes.data_as(ctypes.c_void_p), mel.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(win, ofe.periodic_hann(400))
    ref = ofe.mel_matrix(64, 257, 16000, 125.0, 7500.0)
    np.testing.assert_allclose(mel, ref, rtol=0, atol=1e-15)
    assert np.array_equal(mel != 0, ref != 0)
    n = lib.mla_logmel_table_floats()
    tab = np.zeros(n, dtype=np.float32)
    assert lib.mla_logmel_build_tables(tab.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(tab[:400], win.astype(np.float32)) and not tab[400:512].any()
    m = np.arange(256)
    np.testing.assert_allclose(tab[512:1024:2], np.cos(2 * np.pi * m / 256), atol=1e-7)
    np.testing.assert_allclose(tab[513:1024:2], -np.sin(2 * np.pi * m / 256), atol=1e-7)
    # sparse per-lane mel rows reproduce the dense matrix (weights are stored halved)
    starts = tab[1536:1600].view(np.int32).reshape(16, 4)
    rows = tab[1600:1600 + 16 * 52].reshape(16, 52)
    dense = np.zeros((257, 64))
    counts = (8, 8, 12, 20)
    for lane in range(16):
        bands = (lane, 31 - lane, 32 + lane, 63 - lane)
        first = 0
        for s in range(4):
            assert 4 <= starts[lane, s] and starts[lane, s] % 4 == 0 and starts[lane, s] + counts[s] <= 256
            dense[starts[lane, s]:starts[lane, s] + counts[s], bands[s]] = 2.0 * rows[lane, first:first + counts[s]]
            first += counts[s]
    np.testing.assert_allclose(dense, ref, rtol=1e-7, atol=0)


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostsim") / "hostsim.so")
    src = os.path.join(ROOT, PKG, "csrc", "logmel_hostsim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    lib.hostsim_examples.restype = ctypes.c_int64
    lib.hostsim_examples.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    return lib


def mel_domain_close(got, ref, rel=2e-5, floor=2e-6):
    """|mel - mel_ref| <= rel*mel_ref + floor*max(mel_ref of the frame): float32 dynamic range
    (about -115 dB below the frame's strongest band), see DESIGN.md "front-end tolerance"."""
    g, r = np.exp(got.astype(np.float64)) - 0.01, np.exp(ref) - 0.01
    bound = rel * r + floor * r.max(axis=-1, keepdims=True) + 1e-9
    return bool(np.all(np.abs(g - r) <= bound)), float(np.max(np.abs(g - r) / bound))


def test_kernel_math_on_host_matches_oracle(hostsim, mk):
    for name, wav in mk.test_waveforms().items():
        if wav.ndim > 1:
            wav = wav.mean(axis=1)
        x = np.ascontiguousarray(wav.astype(np.float32))
        ref = ofe.waveform_to_examples(wav)
        out = np.zeros(ref.shape, dtype=np.float32)
        n = hostsim.hostsim_examples(x.ctypes.data_as(ctypes.c_void_p), len(x), out.ctypes.data_as(ctypes.c_void_p))
        assert n == ref.shape[0], name
        ok, worst = mel_domain_close(out, ref)
        assert ok, (name, worst)
        if name.startswith(("noise", "stereo", "silence")):       # broadband: log-domain bound
            assert np.abs(out - ref).max() <= 1e-4, name


def test_argument_errors_are_reported_before_any_launch(L):
    """Error behaviour of the C ABI (include/mla_hip.h): negative MLA_E_* codes + a message in mla_last_error(), decided on
    the host before any HIP call -- so it is checkable without a GPU. Zero-sized work returns MLA_OK without touching
    its (null) buffers, like the reference's functions on empty inputs."""
    lib = L.lib()
    lib.mla_last_error.restype = ctypes.c_char_p
    vp = ctypes.c_void_p
    fake = vp(0x1000)                                # aligned, never dereferenced: every call below fails validation first
    E_ARG, E_SHAPE, E_SHORT, E_DTYPE = -1, -2, -3, -5

    def expect(code, rc, needle=None):
        assert rc == code, (rc, lib.mla_last_error())
        if needle:
            assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    # front-end: reference raises ValueError for n < 240 (negative frame count)
    expect(E_SHORT, lib.mla_logmel_examples(fake, L.F32, 1, 239, 239, fake, fake, L.F32, None), "239")
    expect(E_DTYPE, lib.mla_logmel_examples(fake, 7, 1, 16000, 16000, fake, fake, L.F32, None))
    expect(E_DTYPE, lib.mla_logmel_examples(fake, L.F32, 1, 16000, 16000, fake, fake, L.I16, None))
    expect(E_ARG, lib.mla_logmel_examples(None, L.F32, 1, 16000, 16000, fake, fake, L.F32, None), "null")
    expect(E_ARG, lib.mla_logmel_examples(fake, L.F32, 1, 16000, 15999, fake, fake, L.F32, None))      # stride < n_samples
    expect(E_ARG, lib.mla_logmel_examples(fake, L.F32, 1, 16000, 16000, fake, vp(0x1004), L.F32, None))  # out misaligned
    assert lib.mla_logmel_examples(None, L.F32, 0, 16000, 16000, None, None, L.F32, None) == 0          # no waveforms
    assert lib.mla_logmel_examples(None, L.F32, 4, 15599, 15599, None, None, L.F32, None) == 0          # 0 examples each
    expect(E_ARG, lib.mla_mono_mix(fake, L.F32, 100, 0, fake, None))
    expect(E_DTYPE, lib.mla_mono_mix(fake, L.BF16, 100, 2, fake, None))
    assert lib.mla_mono_mix(None, L.F32, 0, 2, None, None) == 0
    # GEMM / conv
    expect(E_ARG, lib.mla_linear(fake, 64, fake, 64, None, fake, 64, -1, 64, 64, L.F32, L.F32, 0, None))
    expect(E_SHAPE, lib.mla_linear(fake, 66, fake, 66, None, fake, 64, 8, 64, 66, L.F32, L.F32, 0, None), "16-byte rows")
    expect(E_DTYPE, lib.mla_linear(fake, 64, fake, 64, None, fake, 64, 8, 64, 64, L.F32, L.BF16, 0, None))
    expect(E_ARG, lib.mla_linear(vp(0x1008), 64, fake, 64, None, fake, 64, 8, 64, 64, L.F32, L.F32, 0, None), "aligned")
    assert lib.mla_linear(None, 64, None, 64, None, None, 64, 0, 64, 64, L.F32, L.F32, 0, None) == 0
    expect(E_DTYPE, lib.mla_vggish_conv(2, fake, fake, fake, fake, 4, 9, None))
    expect(E_ARG, lib.mla_vggish_conv(2, None, fake, fake, fake, 4, L.BF16, None))
    assert lib.mla_vggish_conv(2, None, None, None, None, 0, L.BF16, None) == 0
    rc = lib.mla_vggish_conv(9, fake, fake, fake, fake, 4, L.BF16, None)
    assert rc in (E_ARG, E_SHAPE) and b"layer" in lib.mla_last_error()
    # training kernels: pooled ReLU backward needs even H, W in BOTH forms (an odd size would leave the last row / column of dZ
    # unwritten); un-pooled it does not, and zero images are a no-op
    expect(E_SHAPE, lib.mla_relu_pool_bwd(fake, fake, fake, 2, 13, 8, 64, 1, None), "even")
    expect(E_SHAPE, lib.mla_relu_pool_bwd(fake, fake, fake, 2, 12, 7, 64, 1, None), "even")
    expect(E_SHAPE, lib.mla_relu_pool_bwd_bias(fake, fake, fake, 2, 13, 8, 64, 1, fake, fake, None), "even")
    expect(E_ARG, lib.mla_relu_pool_bwd(None, fake, fake, 2, 12, 8, 64, 1, None))
    assert lib.mla_relu_pool_bwd(fake, fake, fake, 0, 13, 7, 64, 0, None) == 0
    assert lib.mla_relu_pool_bwd(fake, fake, fake, 0, 12, 8, 64, 1, None) == 0
    # the bf16 forms: 8 channels per lane and a fixed grid whose stride must be a multiple of C / 8 (C = 24: 262 144 % 3 != 0); even
    # H, W; the bias gradient needs the workspace of double slots
    for bad_c in (24, 12, 0):
        expect(E_SHAPE, lib.mla_relu_pool_bwd_bf16(fake, L.BF16, fake, L.BF16, fake, 2, 12, 8, bad_c, 1, fake, fake, None), "channel count")
        expect(E_SHAPE, lib.mla_pool_bwd_codes_bf16(fake, fake, fake, 2, 12, 8, bad_c, fake, fake, None), "channel count")
    expect(E_SHAPE, lib.mla_relu_pool_bwd_bf16(fake, L.BF16, fake, L.BF16, fake, 2, 13, 8, 64, 1, fake, fake, None), "even")
    expect(E_SHAPE, lib.mla_relu_pool_bwd_bf16(fake, L.BF16, fake, L.BF16, fake, 2, 12, 7, 64, 1, None, None, None), "even")
    expect(E_SHAPE, lib.mla_pool_bwd_codes_bf16(fake, fake, fake, 2, 13, 8, 64, fake, fake, None), "even")
    expect(E_SHAPE, lib.mla_pool_bwd_codes_bf16(fake, fake, fake, 2, 12, 7, 64, None, None, None), "even")
    expect(E_ARG, lib.mla_relu_pool_bwd_bf16(fake, L.BF16, fake, L.BF16, fake, 2, 12, 8, 64, 1, None, fake, None), "workspace")
    expect(E_ARG, lib.mla_relu_pool_bwd_bf16(fake, L.BF16, fake, L.BF16, fake, 2, 12, 8, 64, 0, None, fake, None), "workspace")
    expect(E_ARG, lib.mla_pool_bwd_codes_bf16(fake, fake, fake, 2, 12, 8, 64, None, fake, None), "workspace")
    expect(E_DTYPE, lib.mla_relu_pool_bwd_bf16(fake, L.BF16, fake, L.F32, fake, 2, 12, 8, 64, 1, fake, fake, None))
    # BatchNorm backward, second stage: the channel layout is validated exactly as in the first (mla_bn_bwd_sums)
    cd = ctypes.c_double

    def bwd_sums(rows, cols, mode, period, act=0, yout=None):
        return lib.mla_bn_bwd_sums(fake, cols, fake, cols, yout, cols, act, 1.0, rows, cols, mode, period, fake, fake, 1e-5, fake, fake, None)

    def bwd_apply(rows, cols, mode, period, act=0, yout=None, count=1.0):
        return lib.mla_bn_bwd_apply(fake, cols, fake, cols, yout, cols, act, 1.0, rows, cols, mode, period, fake, fake, fake, 1e-5,
                                    fake, fake, cd(count), fake, cols, 0, fake, fake, None)

    for rows, cols, mode, period, code in ((20, 8, 0, 0, E_SHAPE),          # period 0: r % period on the device
                                           (20, 8, 0, -1, E_SHAPE), (20, 8, 0, 65, E_SHAPE),      # more than 64 channels
                                           (20, 8, 0, 3, E_SHAPE),           # rows not a multiple of the period
                                           (20, 65, 1, 0, E_SHAPE),          # mode 1: columns are channels
                                           (20, 8, 2, 10, E_SHAPE), (20, 8, -1, 10, E_SHAPE),     # no such mode
                                           (0, 8, 0, 10, E_ARG), (-10, 8, 0, 10, E_ARG), (20, 0, 1, 0, E_ARG)):
        expect(code, bwd_sums(rows, cols, mode, period))
        expect(code, bwd_apply(rows, cols, mode, period))
    expect(E_ARG, bwd_sums(20, 8, 0, 10, act=1), "forward output")
    expect(E_ARG, bwd_apply(20, 8, 0, 10, act=1), "forward output")
    expect(E_ARG, bwd_apply(20, 8, 0, 10, count=0.0))
    expect(E_ARG, lib.mla_bn_bwd_apply(fake, 8, fake, 8, None, 8, 0, 1.0, 20, 8, 0, 10, fake, fake, fake, 1e-5, fake, fake, cd(1.0), fake, 8,
                                       0, fake, None, None), "go together")
    # an uncompiled wgrad shape is refused by the dispatcher, not launched
    expect(E_SHAPE, lib.mla_conv_wgrad(fake, fake, 3, 24, 16, 64, 128, fake, 1 << 30, fake, None), "not compiled")


def test_dropin_front_end_argument_errors_are_reported_before_any_launch(L):
    """The stand-alone entries of csrc/stft_generic.hip (mla_stft_magnitude, mla_mel_log, mla_dataset_frames, mla_postprocess,
    mla_resample, mla_resample_length): every refusal is decided on the host, and work of zero size returns MLA_OK without a launch."""
    lib = L.lib()
    vp = ctypes.c_void_p
    fake = vp(0x1000)                                # aligned, never dereferenced: no call below reaches a launch
    E_ARG, E_SHAPE, E_SHORT = -1, -2, -3

    def expect(code, rc, needle=None):
        assert rc == code, (rc, lib.mla_last_error())
        if needle:
            assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    def stft(n, win, hop, fft, signal=fake, window=fake, twiddle=fake, out=fake):
        return lib.mla_stft_magnitude(signal, n, window, twiddle, win, hop, fft, out, None)

    for fft in (3, 6, 400, 1000, 4095):
        expect(E_SHAPE, stft(16000, 2, 1, fft), "power-of-two")
    expect(E_SHAPE, stft(16000, 400, 160, 256), "power-of-two")              # fft < win
    expect(E_SHAPE, stft(16000, 2, 1, 1))                                    # fft 1 is a power of two, below 2
    expect(E_SHAPE, stft(16000, 400, 160, 8192), "4096")                     # above kMaxFft
    expect(E_SHAPE, stft(16000, 0, 160, 512))
    expect(E_SHAPE, stft(16000, 400, 0, 512))
    for null in ("signal", "window", "twiddle", "out"):
        expect(E_ARG, stft(16000, 400, 160, 512, **{null: None}), "null")
    assert stft(399, 400, 160, 512) == 0 and stft(0, 1, 1, 2) == 0           # n < win: zero frames

    def mel_log(frames, bins, bands, spec=fake, mel=fake, out=fake):
        return lib.mla_mel_log(spec, mel, frames, bins, bands, 0.01, out, None)

    expect(E_ARG, mel_log(3, 0, 64))
    expect(E_ARG, mel_log(3, 257, 0))
    expect(E_ARG, mel_log(-1, 257, 64))
    expect(E_ARG, mel_log(3, 257, 64, spec=None))
    expect(E_ARG, mel_log(3, 257, 64, mel=None))
    expect(E_ARG, mel_log(3, 257, 64, out=None))
    assert mel_log(0, 257, 64) == 0

    def frames(clips, ex, n_frames, frame_len, stride, examples=fake, out=fake):
        return lib.mla_dataset_frames(examples, clips, ex, n_frames, frame_len, stride, out, None)

    expect(E_ARG, frames(1, 5, 10, 96, 32), "at most 4")
    expect(E_ARG, frames(1, -1, 10, 96, 32))
    expect(E_ARG, frames(-1, 4, 10, 96, 32))
    expect(E_ARG, frames(1, 4, 0, 96, 32))
    expect(E_ARG, frames(1, 4, 10, 0, 32))
    expect(E_ARG, frames(1, 4, 10, 96, -1))
    expect(E_ARG, frames(1, 4, 10, 96, 32, out=None))
    expect(E_SHAPE, frames(1, 4, 10, 97, 32), "384")                         # (10 - 1) * 32 + 97 = 385
    expect(E_SHAPE, frames(1, 4, 385, 1, 1), "384")
    expect(E_SHAPE, frames(1, 4, 65537, 1, 65536), "384")                    # 65536 * 65536 wraps to 0 in 32 bits
    expect(E_SHAPE, frames(1, 4, 2, 1, 2147483647), "384")
    expect(E_ARG, frames(1, 4, 10, 96, 32, examples=None), "null examples")
    assert frames(0, 0, 10, 96, 32, examples=None) == 0                       # null examples go with ex_per_clip = 0
    assert frames(0, 4, 10, 96, 32) == 0

    def postprocess(rows, x=fake, ev=fake, mu=fake, out=fake):
        return lib.mla_postprocess(x, ev, mu, rows, out, None)

    assert postprocess(0) == 0
    expect(E_ARG, postprocess(-1))
    for null in ("x", "ev", "mu", "out"):
        expect(E_ARG, postprocess(3, **{null: None}))

    def resample(n_in, sr_in, sr_out, n_out, nwin=32769, num_table=512, x=fake, win=fake, delta=fake, y=fake):
        return lib.mla_resample(x, n_in, sr_in, sr_out, win, delta, nwin, num_table, y, n_out, None)

    expect(E_SHAPE, resample(44100, 44100.0, 16000.0, 16001), "n_out")
    expect(E_SHAPE, resample(44100, 44100.0, 16000.0, 15999), "n_out")
    expect(E_SHORT, resample(1, 44100.0, 16000.0, 0), "too short")
    expect(E_SHORT, resample(0, 44100.0, 16000.0, 0))
    expect(E_SHAPE, resample(2048, 16000.0 * 1024, 16000.0, 2), "resolution")  # int(512 / 1024) = 0 table entries per input sample
    expect(E_ARG, resample(44100, 0.0, 16000.0, 16000))
    expect(E_ARG, resample(44100, 44100.0, -1.0, 16000))
    expect(E_ARG, resample(-1, 44100.0, 16000.0, 0))
    expect(E_ARG, resample(44100, 44100.0, 16000.0, 16000, nwin=1))
    expect(E_ARG, resample(44100, 44100.0, 16000.0, 16000, num_table=0))
    for null in ("x", "win", "delta", "y"):
        expect(E_ARG, resample(44100, 44100.0, 16000.0, 16000, **{null: None}), "null")
    assert lib.mla_resample_length(44100, 44100.0, 16000.0) == 16000 and lib.mla_resample_length(3, 44100.0, 16000.0) == 1
    assert lib.mla_resample_length(1, 44100.0, 16000.0) == 0
    for n_in, a, b in ((100, 0.0, 16000.0), (100, 44100.0, 0.0), (100, -44100.0, 16000.0), (100, float("nan"), 16000.0), (-1, 44100.0, 16000.0)):
        assert lib.mla_resample_length(n_in, a, b) == -1


def _build_c_example(L, tmp_path):
    """gcc -std=c99 on examples/c_abi_logmel.c against include/mla_hip.h + libmla_hip.so: the header is plain C."""
    L.lib()
    exe = str(tmp_path / "c_abi_logmel")
    pkg = os.path.join(ROOT, PKG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "c_abi_logmel.c"), "-L" + pkg, "-lmla_hip", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def test_c_host_compiles_against_the_header(L, tmp_path):
    assert os.path.exists(_build_c_example(L, tmp_path))


@pytest.mark.gpu
def test_c_host_runs(L, tmp_path):
    """The plain-C host (no Python, no torch in the process) produces examples and sees the reference's short-input error."""
    out = subprocess.run([_build_c_example(L, tmp_path)], check=True, capture_output=True, text=True).stdout
    assert "examples (40, 96, 64)" in out and "rc -3" in out, out
