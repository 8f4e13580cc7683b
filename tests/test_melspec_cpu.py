"""The ResNet branch's mel-dB front-end without a GPU: the float64 restatement (tests/librosa_restated.py) anchored to the
values librosa documents, the library's host-built tables and the kernel arithmetic simulated on the host
(csrc/melspec_hostsim.cpp) against it, the C ABI's argument errors, and the refusals that stay pinned."""

import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import librosa_restated as R
from conftest import PKG, ROOT

SR = 22050

# Power-domain tolerance, |S - S_ref| <= REL * S_ref + FLOOR * max_band(S_ref of the frame) with S = 10^(D / 10): four times what an
# independent float32 evaluation of the restatement (R.mel_power_f32: pocketfft on float32 frames, float32 power, mel product and dB
# round trip) reaches against float64 on the waveforms below, REL_BASE = 3.8e-6 and FLOOR_BASE = 5.5e-10 (DESIGN.md section 5,
# "mel-dB front-end tolerance"). test_tolerance_constants_are_four_times_the_float32_baseline re-measures the baseline. Measured worst
# error / bound: host simulation 0.33, MI355X 0.26.
REL_BASE, FLOOR_BASE = 3.8e-6, 5.5e-10
REL, FLOOR = 4 * REL_BASE, 4 * FLOOR_BASE

# (n_samples, hop, n_mels): the GPU tests' small shapes; the baseline and the host simulation run on the same ones
SHAPES = ((1025, 98, 224), (4096, 128, 32), (5000, 98, 224), (5000, 39, 224))


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("melspec_hostsim") / "melspec_hostsim.so")
    src = os.path.join(ROOT, PKG, "csrc", "melspec_hostsim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    lib.hostsim_melspec_db.restype = ctypes.c_int64
    lib.hostsim_melspec_db.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_int64, ctypes.c_float,
                                       ctypes.c_void_p]
    return lib


def test_mel_scale_matches_librosa_documented_values():
    assert abs(float(R.hz_to_mel(60)) - 0.9) <= 1e-12
    np.testing.assert_allclose(R.hz_to_mel([110, 220, 440]), [1.65, 3.3, 6.6], rtol=0, atol=1e-12)
    np.testing.assert_allclose(R.mel_to_hz([1, 2, 3, 4, 5]), [66.667, 133.333, 200.0, 266.667, 333.333], rtol=0, atol=1e-3)
    f = R.mel_frequencies(n_mels=40, fmin=0, fmax=11025)
    assert f.shape == (40,)
    np.testing.assert_allclose(f[:4], [0.0, 85.317, 170.635, 255.952], rtol=0, atol=1e-3)
    assert abs(f[12] - 1024.856) <= 1e-3 and abs(f[-1] - 11025.0) <= 1e-3
    # the scale is continuous at 1 kHz and the two directions invert each other
    np.testing.assert_allclose(R.mel_to_hz(R.hz_to_mel([0.0, 999.0, 1000.0, 1001.0, 11025.0])), [0.0, 999.0, 1000.0, 1001.0, 11025.0], rtol=1e-12)


def test_filterbank_shape_and_no_empty_filter():
    m = R.mel_filters(SR, 224)
    assert m.shape == (224, 1025) and (m >= 0).all()
    assert ((m != 0).sum(axis=1) >= 1).all()
    mel_f = R.mel_frequencies(226, 0.0, SR / 2)
    assert 29.5 <= (mel_f[2:] - mel_f[:-2]).min() <= 29.7 and abs(SR / 2 / 1024 - 10.77) < 0.01
    assert ((m != 0).sum(axis=0) <= 2).all()               # a bin lies inside at most two triangles


def test_frame_counts_and_split_offsets():
    P = importlib.import_module(PKG + ".params")
    ds = importlib.import_module(PKG + ".dataset")
    assert (P.SR_RESNET, P.SAMPLES_NUM_RESNET, P.MAX_SECONDS) == (22050, 88200, 4)
    n = 88200
    hop = R.hop_length(n, 224, True)
    assert hop == 98 == ds.resnet_hop_length(n, 224, True) and R.num_frames(n, hop) == 901
    step = R.split_step(901, 10, 224, True)
    assert step == 75 and 9 * step + 224 == 899 <= 901         # the last image ends at column 899 (exclusive)
    hop = R.hop_length(n, 224, False)
    assert hop == 39 == ds.resnet_hop_length(n, 224, False) and R.num_frames(n, hop) == 2262
    assert R.split_step(2262, 10, 224, False) == 224 and 10 * 224 <= 2262
    spec = np.arange(3 * 901, dtype=np.float64).reshape(3, 901)
    fr = R.split(spec, 10, 224, True)
    assert fr.shape == (10, 3, 224) and [int(f[0, 0]) for f in fr] == [75 * t for t in range(10)] and int(fr[-1][0, -1]) + 1 == 899
    # the package's split (zero-copy views) is the same gather
    for overlap, width in ((True, 901), (False, 2262)):
        spec = np.random.default_rng(0).standard_normal((4, width))
        assert np.array_equal(ds.split(torch.from_numpy(spec), 10, 224, 4, overlap).numpy(), R.split(spec, 10, 224, overlap))


def _tables(L, sr, n_mels):
    lib = L.lib()
    n = lib.mla_melspec_table_floats(float(sr), n_mels)
    assert n > 0
    tab = np.zeros(n, dtype=np.float32)
    assert lib.mla_melspec_build_tables(float(sr), n_mels, tab.ctypes.data_as(ctypes.c_void_p)) == 0
    return tab


@pytest.mark.parametrize("n_mels", [224, 32])
def test_host_tables_match_restatement(L, n_mels):
    tab = _tables(L, SR, n_mels)
    assert np.array_equal(tab[:2048], R.hann_periodic().astype(np.float32))
    k = np.arange(1536)
    np.testing.assert_allclose(tab[2048:5120:2], np.cos(2 * np.pi * k / 2048), rtol=0, atol=6e-8)
    np.testing.assert_allclose(tab[2049:5120:2], -np.sin(2 * np.pi * k / 2048), rtol=0, atol=6e-8)
    meta = tab[5120:5120 + 3 * n_mels].view(np.int32).reshape(n_mels, 3)
    weights = tab[5120 + 3 * n_mels:]
    ref = R.mel_filters(SR, n_mels)
    assert len(weights) == meta[:, 1].sum() == np.count_nonzero(ref) and len(weights) <= 2 * 1025
    assert np.array_equal(meta[:, 2], np.concatenate([[0], np.cumsum(meta[:, 1])[:-1]]))
    dense = np.zeros((n_mels, 1025), dtype=np.float32)
    for b, (first, bins, off) in enumerate(meta):
        assert bins >= 1 and 0 <= first and first + bins <= 1025
        dense[b, first:first + bins] = weights[off:off + bins]
    assert np.array_equal(dense != 0, ref != 0), "zeros are exact"
    np.testing.assert_allclose(dense.astype(np.float64), ref, rtol=3 * 2.0 ** -24, atol=0)     # computed in double, rounded once


def test_table_builder_rejects_bad_configurations(L):
    lib = L.lib()
    assert lib.mla_melspec_table_floats(0.0, 224) == -1 and lib.mla_melspec_table_floats(22050.0, 0) == -1
    assert lib.mla_melspec_table_floats(22050.0, 1025) == -1
    buf = np.zeros(8, dtype=np.float32)
    assert lib.mla_melspec_build_tables(22050.0, 0, buf.ctypes.data_as(ctypes.c_void_p)) == -1
    assert lib.mla_melspec_build_tables(22050.0, 224, None) == -1
    assert lib.mla_melspec_frames(88200, 98) == 901 and lib.mla_melspec_frames(88200, 39) == 2262
    assert lib.mla_melspec_frames(88200, 0) == -1 and lib.mla_melspec_frames(-1, 98) == -1
    assert lib.mla_melspec_workspace_bytes(3, 88200, 98) == 3 * 57 * 4 and lib.mla_melspec_workspace_bytes(1, 88200, 0) == -1


@pytest.fixture(scope="module")
def references():
    """float64 mel powers of every waveform at every small shape, computed once."""
    return {(name, shape): R.mel_power(R.waveform(name, shape[0]), SR, shape[2], shape[1]) for name in R.WAVEFORMS for shape in SHAPES}


def test_tolerance_constants_are_four_times_the_float32_baseline(references):
    pairs = [(R.mel_power_f32(R.waveform(name, n), SR, n_mels, hop), ref) for (name, (n, hop, n_mels)), ref in references.items()]
    rel, floor = R.baseline_constants(pairs)
    print("float32 baseline: rel %.3g floor %.3g" % (rel, floor))
    # the recorded constants are this measurement rounded up; pocketfft builds may differ in the last digit, not by a quarter
    assert rel <= REL_BASE <= 1.25 * rel and floor <= FLOOR_BASE <= 1.25 * floor, (rel, floor)
    assert (REL, FLOOR) == (4 * REL_BASE, 4 * FLOOR_BASE)


def run_hostsim(hostsim, x, hop, n_mels):
    frames = R.num_frames(len(x), hop)
    out = np.full((n_mels, frames), np.nan, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    got = hostsim.hostsim_melspec_db(x.ctypes.data_as(ctypes.c_void_p), len(x), hop, float(SR), n_mels, R.AMIN,
                                     out.ctypes.data_as(ctypes.c_void_p))
    assert got == frames
    return out


def test_kernel_math_on_host_matches_restatement(hostsim, references):
    worst = 0.0
    for (name, (n, hop, n_mels)), ref in references.items():
        D = run_hostsim(hostsim, R.waveform(name, n), hop, n_mels)
        assert np.isfinite(D).all() and D.shape == ref.shape
        S = R.db_to_power(D)
        ok, ratio = R.power_close(S, ref, REL, FLOOR)
        worst = max(worst, ratio)
        assert ok, (name, n, hop, n_mels, ratio)
        for sl in (slice(0, 11), slice(-11, None)):          # the frames that read reflected samples pass on their own
            assert R.power_close(S[:, sl], ref[:, sl], REL, FLOOR)[0], (name, n, hop, sl)
        if name == "silence":
            assert np.abs(D + 100.0).max() <= 1e-4
    print("host simulation: worst error / bound %.3f" % worst)


def test_host_simulation_run_boundaries(hostsim):
    """hop 512 leaves room for 5 frames per run instead of 16 and hop 3000 for one: the same values as the restatement."""
    x = R.waveform("noise", 12000)
    for hop in (512, 3000):
        D = run_hostsim(hostsim, x, hop, 32)
        assert R.power_close(R.db_to_power(D), R.mel_power(x, SR, 32, hop), REL, FLOOR)[0], hop


def test_burst_clip_sits_partly_on_the_floor():
    """The GPU clip-and-gather test uses this clip: between 10 % and 90 % of its elements are at max - 80 dB, so a test where nothing
    or everything is clipped cannot pass for the wrong reason."""
    D = R.melspectrogram_db(R.waveform("burst", 88200), SR, 224, 98)
    on_floor = float((D == D.max() - 80.0).mean())
    print("burst clip: %.1f %% of the elements on the floor" % (100 * on_floor))
    assert 0.10 <= on_floor <= 0.90, on_floor
    silent = R.melspectrogram_db(np.zeros(88200), SR, 224, 98)
    assert (silent == -100.0).all()


def test_argument_errors_are_reported_before_any_launch(L):
    lib = L.lib()
    vp = ctypes.c_void_p
    fake = vp(0x1000)                                # never dereferenced: every call below fails validation first
    E_ARG, E_SHAPE, E_SHORT = -1, -2, -3
    cf = ctypes.c_float

    def expect(code, rc, needle=None):
        assert rc == code, (rc, lib.mla_last_error())
        if needle:
            assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    def db(pcm=fake, clips=1, n=88200, stride=88200, hop=98, n_mels=224, amin=1e-10, tab=fake, out=fake, ws=fake):
        return lib.mla_melspec_db(pcm, clips, n, stride, hop, n_mels, cf(amin), tab, out, ws, None)

    def images(d=fake, ws=fake, clips=1, n=88200, hop=98, n_mels=224, top_db=80.0, n_images=10, w=224, stride=75, out=fake):
        return lib.mla_melspec_images(d, ws, clips, n, hop, n_mels, cf(top_db), n_images, w, stride, out, None)

    expect(E_SHORT, db(n=1024, stride=1024), "1025")
    expect(E_SHORT, images(n=1024), "1025")
    expect(E_ARG, db(hop=0), "hop")
    expect(E_ARG, images(hop=0), "hop")
    expect(E_ARG, db(n_mels=0), "n_mels")
    expect(E_ARG, db(n_mels=1025), "n_mels")
    expect(E_ARG, db(stride=88199), "stride")
    expect(E_ARG, db(amin=0.0), "amin")
    expect(E_ARG, db(clips=-1))
    for null in ("pcm", "tab", "out", "ws"):
        expect(E_ARG, db(**{null: None}), "null")
    expect(E_SHAPE, images(stride=76), "leave")                      # 9 * 76 + 224 = 908 > 901
    expect(E_SHAPE, images(w=902, n_images=1, stride=0), "leave")
    expect(E_SHAPE, images(hop=39, n_images=11, stride=224), "leave")   # 11 * 224 > 2262
    expect(E_ARG, images(n_images=0))
    expect(E_ARG, images(top_db=-1.0), "top_db")
    for null in ("d", "ws", "out"):
        expect(E_ARG, images(**{null: None}), "null")
    assert db(pcm=None, clips=0, tab=None, out=None, ws=None) == 0    # no clips: nothing to do
    assert images(d=None, ws=None, out=None, clips=0) == 0


def test_pinned_refusals_still_hold():
    ds = importlib.import_module(PKG + ".dataset")
    M = importlib.import_module(PKG + ".model")
    with pytest.raises(NotImplementedError):
        ds.create_spec(np.zeros(64000), "vggish", 16000, 64000, 96, 64, True, True)
    conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    rn = M.Ensemble("repeat", conf, [2, 1], "cpu")
    with pytest.raises(NotImplementedError):
        rn.forward_waveforms(torch.zeros(1, 160000))
    vg = M.Ensemble("repeat", dict(conf, cnn_type="vggish"), [2, 1], "cpu")
    with pytest.raises(NotImplementedError, match="forward_waveforms"):
        vg.forward_clips(torch.zeros(1, 88200))
