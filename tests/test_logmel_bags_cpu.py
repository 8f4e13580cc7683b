"""Ragged recordings -> VGGish bags (csrc/logmel.hip logmel_bags_kernel, csrc/logmel_bags_core.h) without a GPU: the kernel's work items
simulated on the host (csrc/logmel_bags_hostsim.cpp: logmel_core.h's phases, the shared item / window / offset arithmetic) against the
float64 chain oracle.dataset_frames.split(create_spec_native(x)), which tests/golden/dataset.npz pins to the reference's own functions;
the C ABI's argument errors; the Python refusals that come before the device is touched.

The bound, 1e-4 absolute, is the project's log-mel bound (tests/test_dataset_frames.py). It is applied to broadband input only (uniform
noise of amplitude 0.5): where a mel band is empty, d log = d mel / 0.01 at ln 0.01 and float32 arithmetic moves the value by ~2e-4, so
tonal and upsampled rows are covered by the bit-equality tests of tests/test_logmel_bags_gpu.py instead."""

import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from oracle import dataset_frames as ods
from oracle import frontend as ofe

ROW = 61680                       # 15 600 + 3 * 15 360: all that four examples read
LENGTHS = (240, 15599, 15600, 30959, 30960, 46320, 61679, 61680, 64000, 77039)
CONFIGS = ((10, 32), (4, 96))
TOL = 1e-4


def noise(index, n):
    """Seeded uniform noise of amplitude 0.5 at 16 kHz, float32."""
    return np.random.default_rng(7000 + index).uniform(-0.5, 0.5, size=n).astype(np.float32)


_oracle = {}


def oracle_frames(index, overlap):
    """float64 frames of case `index`, computed once per session, shared with the GPU tests and never modified."""
    key = (index, bool(overlap))
    if key not in _oracle:
        spec = ods.create_spec_native(noise(index, LENGTHS[index]).astype(np.float64))
        fr = np.asarray(ods.split(spec, 10, 96, 64, overlap))
        fr.setflags(write=False)
        _oracle[key] = fr
    return _oracle[key]


def rows_and_counts():
    """Each recording zero-filled into a row of ROW samples, or cut to it; counts from the oracle's example arithmetic."""
    rows = np.zeros((len(LENGTHS), ROW), dtype=np.float32)
    for i, n in enumerate(LENGTHS):
        k = min(n, ROW)
        rows[i, :k] = noise(i, n)[:k]
    return rows, np.array([ofe.num_examples(n) for n in LENGTHS], dtype=np.int32)


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("logmel_bags_hostsim") / "logmel_bags_hostsim.so")
    src = os.path.join(ROOT, PKG, "csrc", "logmel_bags_hostsim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.hostsim_logmel_bags.argtypes = [vp, i64, i64, i64, vp, ci, ci, vp, vp]
    return lib


def test_counts_of_the_cases(L):
    """dataset._bag_counts, which sizes the launch (the library's mla_resample_length and mla_logmel_counts), agrees with the oracle's
    example arithmetic on the cases, at 16 kHz and through a resampled length."""
    ds = importlib.import_module(PKG + ".dataset")
    assert [ofe.num_examples(n) for n in LENGTHS] == [0, 0, 1, 1, 2, 3, 3, 4, 4, 4]
    assert ds._bag_counts(LENGTHS, [16000] * len(LENGTHS)).tolist() == [0, 0, 1, 1, 2, 3, 3, 4, 4, 4]
    assert ds._bag_counts([2 * n for n in LENGTHS], [32000] * len(LENGTHS)).tolist() == [0, 0, 1, 1, 2, 3, 3, 4, 4, 4]
    assert ds._bag_counts([176400, 16000, 66150, 96000], [44100, 8000, 22050, 192000]).tolist() == [4, 2, 3, 0]
    assert ds.SAMPLES_NUM_VGGISH == ROW
    with pytest.raises(ValueError):
        ofe.num_examples(239)
    assert ofe.num_examples(77040) == 5


@pytest.mark.parametrize("n_frames,stride", CONFIGS)
def test_hostsim_writes_every_element_once_and_matches_float64_chain(hostsim, n_frames, stride):
    rows, counts = rows_and_counts()
    B = len(LENGTHS)
    out = np.full((B, n_frames, 64, 96), np.nan, dtype=np.float32)
    writes = np.zeros(out.shape, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert hostsim.hostsim_logmel_bags(p(rows), B, ROW, ROW, p(counts), n_frames, stride, p(out), p(writes)) == 0
    assert (writes == 1).all(), "every element of out is written exactly once"
    worst = 0.0
    for i in range(B):
        ref = oracle_frames(i, overlap=stride == 32)
        assert ref.shape == out[i].shape
        assert np.array_equal(out[i] == 0.0, ref == 0.0), (LENGTHS[i], "zero pattern")
        err = float(np.abs(out[i].astype(np.float64) - ref).max())
        worst = max(worst, err)
        print("length %d (%d examples), (%d, %d): |d| %.3g" % (LENGTHS[i], counts[i], n_frames, stride, err))
        assert err <= TOL, (LENGTHS[i], err)
    print("host simulation, (%d, %d): worst |d| %.3g (bound %.3g)" % (n_frames, stride, worst, TOL))


def test_hostsim_refuses_what_the_kernel_refuses(hostsim):
    rows, counts = rows_and_counts()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros((1, 10, 64, 96), dtype=np.float32)
    writes = np.zeros(out.shape, dtype=np.int32)
    assert hostsim.hostsim_logmel_bags(p(rows), 1, ROW, ROW, p(counts), 10, 96, p(out), p(writes)) == -1
    five = np.array([5], dtype=np.int32)
    assert hostsim.hostsim_logmel_bags(p(rows), 1, ROW, ROW, p(five), 10, 32, p(out), p(writes)) == -2
    four = np.array([4], dtype=np.int32)
    assert hostsim.hostsim_logmel_bags(p(rows), 1, ROW - 1, ROW, p(four), 10, 32, p(out), p(writes)) == -2
    assert not writes.any()


def test_argument_errors_are_reported_before_any_launch(L):
    lib = L.lib()
    assert "mla_logmel_bags" in L.declared_symbols()
    vp = ctypes.c_void_p
    fake = vp(0x1000)                                    # device pointers: never dereferenced, every call below fails validation first
    E_ARG, E_SHAPE, E_DTYPE = -1, -2, -5

    def bags(pcm=fake, pcm_dtype=0, clips=2, n_samples=ROW, row_stride=ROW, dev_counts=fake, counts=(4, 0), host=True, n_frames=10,
             stride=32, tables=fake, out=fake, out_dtype=0):
        hc = np.array(counts, dtype=np.int32)
        return lib.mla_logmel_bags(pcm, pcm_dtype, clips, n_samples, row_stride, dev_counts, hc.ctypes.data_as(vp) if host else None,
                                   n_frames, stride, tables, out, out_dtype, None)

    def expect(code, rc, needle=None):
        assert rc == code, (rc, lib.mla_last_error())
        if needle:
            assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    for null in ("pcm", "dev_counts", "tables", "out"):
        expect(E_ARG, bags(**{null: None}), "null")
    expect(E_ARG, bags(host=False), "null")
    expect(E_ARG, bags(clips=-1), "bad clips")
    expect(E_ARG, bags(row_stride=ROW - 1), "stride")
    expect(E_ARG, bags(counts=(5, 0)), "clip 0")
    expect(E_ARG, bags(counts=(4, -1)), "clip 1")
    expect(E_ARG, bags(out=vp(0x1004)), "out must be 16-byte aligned")
    expect(E_ARG, bags(dev_counts=vp(0x1002)), "counts must be 4-byte aligned")
    expect(E_ARG, bags(tables=vp(0x1001)), "tables and counts")
    expect(E_ARG, bags(pcm=vp(0x1002)), "pcm misaligned")
    expect(E_SHAPE, bags(n_samples=ROW - 1), "clip 0")                       # 4 examples read 61 680 samples
    expect(E_SHAPE, bags(counts=(0, 1), n_samples=15599), "clip 1")
    for cfg in ((10, 96), (4, 32), (0, 32), (10, 0), (3, 96)):
        expect(E_SHAPE, bags(n_frames=cfg[0], stride=cfg[1]), "only (10, 32) and (4, 96)")
    for code in (1, 4, 7):
        expect(E_DTYPE, bags(pcm_dtype=code), "pcm_dtype")
    for code in (2, 3, 6):
        expect(E_DTYPE, bags(out_dtype=code), "out_dtype")
    assert bags(clips=0, pcm=None, dev_counts=None, host=False, tables=None, out=None) == 0
    assert bags(clips=0, pcm=None, dev_counts=None, host=False, tables=None, out=None, n_frames=4, stride=96, out_dtype=1) == 0


def test_python_errors_come_before_the_device_is_touched(L):
    ds = importlib.import_module(PKG + ".dataset")
    torch = importlib.import_module("torch")
    ok = np.zeros(16000, dtype=np.float32)
    with pytest.raises(ValueError, match=r"recording 1: negative dimensions are not allowed"):
        ds.recordings_to_frames([ok, np.zeros(239, dtype=np.float32)], 16000)
    with pytest.raises(ValueError, match=r"recording 0: could not broadcast input array from shape \(5,96,64\) into shape \(4,96,64\)"):
        ds.recordings_to_frames([np.zeros(77040, dtype=np.float32), ok], 16000)
    with pytest.raises(ValueError, match=r"recording 1: could not broadcast input array from shape \(6,96,64\) into shape \(4,96,64\)"):
        ds.recordings_to_frames([np.zeros(16000, dtype=np.int16), np.zeros(2 * 92400, dtype=np.int16)], [16000, 32000])   # 92 400 at 16 kHz
    # n_res comes from the library's resampled length: int(717 * 16000 / 48000) = 239, int(720 * ...) = 240
    assert L.lib().mla_resample_length(717, 48000.0, 16000.0) == 239 and L.lib().mla_resample_length(720, 48000.0, 16000.0) == 240
    with pytest.raises(ValueError, match=r"recording 0: negative dimensions"):
        ds.recordings_to_frames([np.zeros((717, 2), dtype=np.float32)], [48000])
    # inherited from recordings_to_clips
    with pytest.raises(ValueError, match=r"recording 1: Input signal length=2 is too small to resample from 48000->16000"):
        ds.recordings_to_frames([ok, np.zeros(2, dtype=np.float32)], [44100, 48000])
    with pytest.raises(ValueError, match=r"recording 2: Invalid sample rate"):
        ds.recordings_to_frames([ok, ok, ok], [44100, 22050, 0])
    with pytest.raises(TypeError, match="all int16 or all floating"):
        ds.recordings_to_frames([ok, np.zeros(16000, dtype=np.int16)], 44100)
    with pytest.raises(ValueError, match="2 recordings but 1 rates"):
        ds.recordings_to_frames([ok, ok], [44100])
    with pytest.raises(ValueError, match="recording 0"):
        ds.recordings_to_frames([np.zeros((2, 3, 4), dtype=np.float32)], 44100)
    empty = ds.recordings_to_frames([], [])
    assert tuple(empty.shape) == (0, 10, 1, 64, 96) and empty.dtype == torch.float32
    empty = ds.recordings_to_frames([], 44100, overlap=False, out_dtype=torch.bfloat16)
    assert tuple(empty.shape) == (0, 4, 1, 64, 96) and empty.dtype == torch.bfloat16
    assert tuple(ds.wavfiles_to_frames([]).shape) == (0, 10, 1, 64, 96)
    assert tuple(ds.audiofiles_to_frames([], overlap=False).shape) == (0, 4, 1, 64, 96)


def test_file_errors_come_before_the_device_is_touched(tmp_path):
    import wave
    ds = importlib.import_module(PKG + ".dataset")

    def write(name, n, width=2, rate=16000):
        path = str(tmp_path / name)
        with wave.open(path, "wb") as wf:
            wf.setnchannels(1)
            wf.setsampwidth(width)
            wf.setframerate(rate)
            wf.writeframes(bytes(n * width))
        return path

    short, long_, wide = write("short.wav", 239), write("long.wav", 77040), write("wide.wav", 16000, width=3)
    for fn in (ds.wavfiles_to_frames, ds.audiofiles_to_frames):
        with pytest.raises(ValueError, match=r"recording 0: negative dimensions"):
            fn([short])
        with pytest.raises(ValueError, match=r"recording 1: could not broadcast input array from shape \(5,96,64\)"):
            fn([write("ok.wav", 16000), long_])
    with pytest.raises(AssertionError, match="Bad sample type: 3"):
        ds.wavfiles_to_frames([wide])


def test_native_entries_refuse_the_resnet_branch_and_contiguous_bags():
    M = importlib.import_module(PKG + ".model")
    conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    rn = M.Ensemble("repeat", conf, [2, 1], "cpu")
    rec = [np.zeros(16000, dtype=np.float32)]
    with pytest.raises(NotImplementedError, match="forward_recordings_native"):
        rn.forward_recordings_native(rec, [16000])
    with pytest.raises(NotImplementedError, match="forward_wavfiles_native"):
        rn.forward_wavfiles_native(["nothing.wav"])
    with pytest.raises(NotImplementedError, match="forward_audiofiles_native"):
        rn.forward_audiofiles_native(["nothing.wav"])
    vg = M.Ensemble("repeat", dict(conf, cnn_type="vggish"), [2, 1], "cpu")
    with pytest.raises(ValueError, match="forward_recordings_native: overlap=False"):
        vg.forward_recordings_native(rec, [16000], overlap=False)
    with pytest.raises(ValueError, match="forward_wavfiles_native: overlap=False"):
        vg.forward_wavfiles_native(["nothing.wav"], overlap=False)
    with pytest.raises(ValueError, match="forward_audiofiles_native: overlap=False"):
        vg.forward_audiofiles_native(["nothing.wav"], overlap=False)
    # the cut-and-zero-fill entries keep refusing VGGish, and now point at the native ones
    with pytest.raises(NotImplementedError, match=r"forward_recordings cuts .* use forward_recordings_native\(\)"):
        vg.forward_recordings(rec, [16000])
