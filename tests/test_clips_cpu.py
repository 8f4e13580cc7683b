"""Recordings -> clips (csrc/clips.hip, csrc/resample_core.h) without a GPU: the kernel's arithmetic simulated on the host workgroup by
workgroup (csrc/clips_hostsim.cpp) against the float64 chain (channel mean rounded to float32, oracle/resample.py, cut, zero fill), the
isolation of the clips of one packed buffer, the C ABI's argument errors, and the Python refusals that come before the device is touched.

The bound, 2e-6 absolute, is tests/test_frontend_gpu.py's for this same arithmetic (double accumulation, one rounding to float32) on
inputs of this amplitude. Parity with resampy itself is unpinned: the oracle restates its published algorithm."""

import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from oracle import resample as oresample

SR_OUT = 22050
TOL = 2e-6
# (sr_in, channels, n_in, n_res = int(n_in * 22050 / sr_in)); 44 100 Hz x 100 frames is shorter than a filter wing
CASES = ((44100, 2, 6001, 3000), (48000, 1, 5000, 2296), (8000, 1, 700, 1929), (11025, 3, 900, 1800), (96000, 1, 9000, 2067),
         (192000, 2, 12000, 1378), (44100, 1, 100, 50), (16000, 1, 2501, 3446))
PASSTHROUGH = ((22050, 1, 1500, 1500), (22050, 1, 3000, 3000))
ALL_CASES = CASES + PASSTHROUGH
SAMPLES_NUMS = (2048, 2000)          # 2000 is no multiple of the 256-output tile


def make_recording(index, int16):
    """Seeded samples of case `index`: uniform in [-0.5, 0.5] float32, or int16 in +-16 000; (n,) for mono, else (n, channels)."""
    _, ch, n, _ = ALL_CASES[index]
    rng = np.random.default_rng(1000 + 2 * index + int(int16))
    x = rng.integers(-16000, 16001, size=(n, ch)).astype(np.int16) if int16 else rng.uniform(-0.5, 0.5, size=(n, ch)).astype(np.float32)
    return x[:, 0].copy() if ch == 1 else x


def mono_f32(x):
    """Mean over the channels in double, times the PCM scale, rounded once to float32."""
    x2 = x.reshape(x.shape[0], -1).astype(np.float64)
    return (x2.sum(axis=1) / x2.shape[1] * (1.0 / 32768.0 if x.dtype == np.int16 else 1.0)).astype(np.float32)


def resampled_f64(x, sr_in):
    """The float64 chain before the cut: the whole recording is the filter's input."""
    m = mono_f32(x).astype(np.float64)
    return m if sr_in == SR_OUT else oresample.resample(m, sr_in, SR_OUT)


def cut_and_fill(y, samples_num):
    row = np.zeros(samples_num, dtype=np.float64)
    k = min(len(y), samples_num)
    row[:k] = y[:k]
    return row


_chain = {}


def chain(index, int16):
    """float64 chain of one case, computed once per session and shared by the CPU and the GPU tests; never modified."""
    key = (index, bool(int16))
    if key not in _chain:
        y = resampled_f64(make_recording(index, int16), ALL_CASES[index][0])
        assert len(y) == ALL_CASES[index][3]
        y.setflags(write=False)
        _chain[key] = y
    return _chain[key]


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


_hostsim = {}


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory):
    """csrc/clips_hostsim.cpp as a ctypes library, built once per session; tests/test_audiofiles_cpu.py imports this fixture."""
    if "lib" not in _hostsim:
        _hostsim["lib"] = build_hostsim(tmp_path_factory)
    return _hostsim["lib"]


def build_hostsim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("clips_hostsim") / "clips_hostsim.so")
    src = os.path.join(ROOT, PKG, "csrc", "clips_hostsim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, ci, cd = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    lib.hostsim_clips_prepare.restype = i64
    lib.hostsim_clips_prepare.argtypes = [vp, ci, i64, vp, vp, vp, vp, vp, cd, i64, vp, ci, ci, vp]
    lib.hostsim_clips_prepare_raw.restype = i64
    lib.hostsim_clips_prepare_raw.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, cd, i64, vp, ci, ci, vp]
    return lib


def pack(recordings, guard=0):
    """(packed, element offsets, frames, channels) of `recordings`, all int16 or all float32, back to back with `guard` elements
    (NaN for float input, 0 for int16) before, between and after them."""
    int16 = recordings[0].dtype == np.int16
    frames = np.array([x.shape[0] for x in recordings], dtype=np.int64)
    channels = np.array([1 if x.ndim == 1 else x.shape[1] for x in recordings], dtype=np.int32)
    sizes = frames * channels
    offsets = (np.concatenate([[0], np.cumsum(sizes + guard)[:-1]]) + guard).astype(np.int64)
    packed = np.full(int((sizes + guard).sum()) + guard, 0 if int16 else np.nan, dtype=np.int16 if int16 else np.float32)
    for x, o, s in zip(recordings, offsets, sizes):
        packed[o:o + s] = x.reshape(-1)
    return packed, offsets, frames, channels


def run_hostsim(hostsim, fe, recordings, rates, samples_num, guard=0, as_bytes=False):
    """Pack `recordings` and run the simulated launch of mla_clips_prepare (element offsets) or, as_bytes, of mla_clips_prepare_raw
    on the same buffer viewed as bytes: offsets x sample size, one format code for all."""
    int16 = recordings[0].dtype == np.int16
    packed, offsets, frames, channels = pack(recordings, guard)
    rates = np.array(rates, dtype=np.float64)
    scales, tab = fe.clips_table_index(rates, float(SR_OUT))
    tables = fe.clips_tables_host(scales)
    nwin = len(tables) // (2 * max(len(scales), 1))
    out = np.full((len(recordings), samples_num), np.nan, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    code, tail = 2 if int16 else 0, (p(rates), p(tab), float(SR_OUT), samples_num, p(tables), nwin if scales else 32769, 512, p(out))
    if as_bytes:
        byte_offsets, formats = offsets * packed.itemsize, np.full(len(recordings), code, dtype=np.int32)
        cap = hostsim.hostsim_clips_prepare_raw(p(packed), len(recordings), p(byte_offsets), p(frames), p(channels), p(formats), *tail)
    else:
        cap = hostsim.hostsim_clips_prepare(p(packed), code, len(recordings), p(offsets), p(frames), p(channels), *tail)
    assert cap >= 0, cap
    return out, cap


def check_rows(got, int16, samples_num, what):
    """The checks every implementation of the batch has to pass: bound, exact zero tail, bit-equal passthrough."""
    worst = 0.0
    for i, (sr_in, _, _, n_res) in enumerate(ALL_CASES):
        y = chain(i, int16)
        ref = cut_and_fill(y, samples_num)
        err = float(np.abs(got[i].astype(np.float64) - ref).max())
        worst = max(worst, err)
        assert np.isfinite(got[i]).all() and err <= TOL, (what, ALL_CASES[i], samples_num, err)
        k = min(n_res, samples_num)
        assert not got[i, k:].any() and not np.signbit(got[i, k:]).any(), (what, ALL_CASES[i], "tail")
        if sr_in == SR_OUT:
            assert np.array_equal(got[i, :k], y[:k].astype(np.float32)), (what, ALL_CASES[i], "passthrough")
    print("%s, samples_num %d, %s: worst |d| %.3g (bound %.3g)" % (what, samples_num, "int16" if int16 else "float32", worst, TOL))


@pytest.mark.parametrize("int16", [False, True])
@pytest.mark.parametrize("samples_num", SAMPLES_NUMS)
def test_kernel_math_on_host_matches_float64_chain(hostsim, fe, samples_num, int16):
    recs = [make_recording(i, int16) for i in range(len(ALL_CASES))]
    got, cap = run_hostsim(hostsim, fe, recs, [c[0] for c in ALL_CASES], samples_num)
    # 192 kHz: int(255 / ratio) + 3 + 2 * (32769 // 58) = 2220 + 3 + 1128 staged floats at the most
    assert cap == 3351
    check_rows(got, int16, samples_num, "host simulation")


@pytest.mark.parametrize("int16", [False, True])
def test_element_and_byte_offsets_give_the_same_rows(hostsim, fe, int16):
    """One kernel serves both entries: the same packed buffer addressed in elements of one format and in bytes with a format code
    per clip gives the same bits. 2000 is no multiple of the tile; the batch has odd element offsets (ALL_CASES)."""
    recs = [make_recording(i, int16) for i in range(len(ALL_CASES))]
    rates = [c[0] for c in ALL_CASES]
    assert any(o % 2 for o in pack(recs)[1])
    typed, cap = run_hostsim(hostsim, fe, recs, rates, 2000)
    raw, cap_raw = run_hostsim(hostsim, fe, recs, rates, 2000, as_bytes=True)
    assert cap == cap_raw == 3351 and np.isfinite(typed).all()
    assert np.array_equal(typed.view(np.uint32), raw.view(np.uint32))


def test_n_res_of_the_cases():
    for sr_in, _, n, n_res in ALL_CASES:
        assert int(n * (float(SR_OUT) / sr_in)) == n_res
    assert 2067 == 8 * 256 + 19 and 100 < 32769 // 256          # one ends 19 past a tile edge; one is shorter than a wing


def test_lds_budget_per_rate(L):
    lib = L.lib()
    # int(255 / ratio) + 3 + 2 * (32769 // int(min(1, ratio) * 512)) floats, ratio = 22050 / sr_in
    for sr_in, floats in ((44100, 769), (48000, 836), (96000, 1673), (192000, 3351), (8000, 223), (16 * SR_OUT, 6131)):
        r = np.array([22050.0, sr_in], dtype=np.float64)
        assert lib.mla_clips_lds_bytes(r.ctypes.data_as(ctypes.c_void_p), 2, float(SR_OUT), 32769, 512) == 4 * floats, sr_in
    r = np.array([22050.0], dtype=np.float64)
    assert lib.mla_clips_lds_bytes(r.ctypes.data_as(ctypes.c_void_p), 1, float(SR_OUT), 32769, 512) == 0
    assert lib.mla_clips_lds_bytes(None, 0, float(SR_OUT), 32769, 512) == 0


def test_clips_of_one_packed_buffer_are_isolated(hostsim, fe):
    order = list(range(len(ALL_CASES)))
    recs = [make_recording(i, False) for i in order]
    rates = [c[0] for c in ALL_CASES]
    base, _ = run_hostsim(hostsim, fe, recs, rates, 2000, guard=64)
    assert np.isfinite(base).all()                       # 64 NaN elements sit before, between and after the clips
    plain, _ = run_hostsim(hostsim, fe, recs, rates, 2000)
    assert np.array_equal(base.view(np.uint32), plain.view(np.uint32))
    perm = [7, 2, 9, 0, 5, 4, 8, 1, 6, 3]
    got, _ = run_hostsim(hostsim, fe, [recs[i] for i in perm], [rates[i] for i in perm], 2000, guard=64)
    for row, i in enumerate(perm):
        assert np.array_equal(got[row].view(np.uint32), base[i].view(np.uint32)), (row, i)


def test_argument_errors_are_reported_before_any_launch(L):
    lib = L.lib()
    assert {"mla_clips_prepare", "mla_clips_lds_bytes"} <= set(L.declared_symbols())
    vp = ctypes.c_void_p
    fake = vp(0x1000)                                    # device pointers: never dereferenced, every call below fails validation first
    E_ARG, E_SHAPE, E_SHORT = -1, -2, -3

    def prepare(packed=fake, dtype=0, packed_elems=10000, clips=2, dev=fake, frames=(1000, 2000), channels=(1, 2), rates=(44100.0, 22050.0),
                offsets=(0, 1000), tab=(0, 0), host=True, sr_out=22050.0, samples_num=2048, tables=fake, n_tables=1, nwin=32769, num_table=512,
                out=fake):
        arrs = [np.array(offsets, dtype=np.int64), np.array(frames, dtype=np.int64), np.array(channels, dtype=np.int32),
                np.array(rates, dtype=np.float64), np.array(tab, dtype=np.int32)]
        hp = [a.ctypes.data_as(vp) if host else None for a in arrs]
        return lib.mla_clips_prepare(packed, dtype, packed_elems, clips, dev, dev, dev, dev, dev, *hp, sr_out, samples_num, tables, n_tables,
                                     nwin, num_table, out, None)

    def expect(code, rc, needle=None):
        assert rc == code, (rc, lib.mla_last_error())
        if needle:
            assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    for null in ("packed", "dev", "tables", "out"):
        expect(E_ARG, prepare(**{null: None}), "null")
    expect(E_ARG, prepare(host=False), "null")
    expect(E_ARG, prepare(clips=-1), "negative")
    expect(E_ARG, prepare(samples_num=-1), "negative")
    expect(E_ARG, prepare(packed_elems=-1), "negative")
    expect(E_ARG, prepare(frames=(-1, 2000)), "clip 0")
    expect(E_ARG, prepare(channels=(1, 0)), "clip 1")
    expect(E_ARG, prepare(rates=(0.0, 22050.0)), "clip 0")
    expect(E_ARG, prepare(rates=(44100.0, -8000.0)), "clip 1")
    expect(E_ARG, prepare(sr_out=0.0), "sr_out")
    expect(E_ARG, prepare(dtype=1), "pcm_dtype")
    expect(E_ARG, prepare(dtype=7), "pcm_dtype")
    expect(E_ARG, prepare(packed_elems=4999), "leave")               # 1000 + 2000 * 2 elements
    expect(E_ARG, prepare(offsets=(-1, 1000)), "leave")
    expect(E_ARG, prepare(tab=(1, 0)), "table")
    expect(E_SHAPE, prepare(rates=(16.0 * 22050 + 1, 22050.0)), "16 x")
    expect(E_SHAPE, prepare(rates=(22050.0 * 513, 22050.0)), "resolution")
    expect(E_SHORT, prepare(frames=(1, 2000)), "too short")
    assert prepare(rates=(16.0 * 22050, 22050.0), clips=0, packed=None, dev=None, host=False, tables=None, out=None) == 0
    assert prepare(clips=0, packed=None, dev=None, host=False, tables=None, out=None, packed_elems=0, n_tables=0) == 0
    r = np.array([16.0 * 22050 + 1], dtype=np.float64)
    assert lib.mla_clips_lds_bytes(r.ctypes.data_as(vp), 1, 22050.0, 32769, 512) == E_SHAPE
    r[0] = 0.0
    assert lib.mla_clips_lds_bytes(r.ctypes.data_as(vp), 1, 22050.0, 32769, 512) == E_ARG
    assert lib.mla_clips_lds_bytes(None, 1, 22050.0, 32769, 512) == E_ARG


def test_python_errors_come_before_the_device_is_touched():
    ds = importlib.import_module(PKG + ".dataset")
    ok = np.zeros(5000, dtype=np.float32)
    with pytest.raises(ValueError, match=r"recording 1: Input signal length=2 is too small to resample from 48000->22050"):
        ds.recordings_to_clips([ok, np.zeros(2, dtype=np.float32)], [44100, 48000])
    with pytest.raises(ValueError, match=r"recording 2: Invalid sample rate"):
        ds.recordings_to_clips([ok, ok, ok], [44100, 22050, 0])
    with pytest.raises(TypeError, match="all int16 or all floating"):
        ds.recordings_to_clips([ok, np.zeros(5000, dtype=np.int16)], 44100)
    with pytest.raises(ValueError, match="2 recordings but 1 rates"):
        ds.recordings_to_clips([ok, ok], [44100])
    with pytest.raises(ValueError, match="recording 0"):
        ds.recordings_to_clips([np.zeros((2, 3, 4), dtype=np.float32)], 44100)
    empty = ds.recordings_to_clips([], [])
    assert tuple(empty.shape) == (0, 88200) and empty.dtype == torch.float32
    assert tuple(ds.recordings_to_clips([], 44100, samples_num=2000).shape) == (0, 2000)
    assert tuple(ds.wavfiles_to_clips([]).shape) == (0, 88200)


def test_forward_recordings_needs_the_resnet_branch():
    M = importlib.import_module(PKG + ".model")
    conf = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    vg = M.Ensemble("repeat", conf, [2, 1], "cpu")
    with pytest.raises(NotImplementedError, match="forward_recordings"):
        vg.forward_recordings([np.zeros(88200, dtype=np.float32)], [22050])
    with pytest.raises(NotImplementedError, match="forward_wavfiles"):
        vg.forward_wavfiles(["nothing.wav"])
