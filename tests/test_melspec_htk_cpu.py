"""The VGGish branch's librosa path (HTK mel-dB of unpadded frames) without a GPU: the float64 restatement
(tests/librosa_htk_restated.py) anchored to the HTK scale and the filterbank's facts, the library's host-built tables and the
wave-per-frame kernel arithmetic simulated on the host (csrc/melspec_wave_hostsim.cpp) against it, the unchanged default tables,
the C ABI's argument errors and the refusals that need no device."""

import ctypes
import hashlib
import importlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import librosa_htk_restated as H
import librosa_restated as R
from conftest import GOLDEN, PKG, ROOT
from test_melspec_cpu import FLOOR, FLOOR_BASE, REL, REL_BASE

# one frame, the last sample short of a second frame, exactly two frames, one frame past a 16-frame run, 20 frames, the workload
LENGTHS = (2048, 2207, 2208, 4608, 5088, 64000)
CFG = (float(H.SR), H.N_MELS, H.FMIN, H.FMAX, 1)


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("melspec_wave_hostsim") / "melspec_wave_hostsim.so")
    src = os.path.join(ROOT, PKG, "csrc", "melspec_wave_hostsim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    lib.hostsim_melspec_nopad_db.restype = ctypes.c_int64
    lib.hostsim_melspec_nopad_db.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_int64,
                                             ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_float, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def mel():
    return H.mel_filters()


@pytest.fixture(scope="module")
def references(mel):
    """float64 mel powers of every waveform at every length, computed once."""
    return {(name, n): H.mel_power(H.clip_waveform(name, n), mel=mel) for name in R.WAVEFORMS for n in LENGTHS}


def test_htk_scale_anchors():
    assert abs(float(H.hz_to_mel(1000.0)) - 1000.0) <= 0.05
    hz = np.array([0.0, 125.0, 700.0, 1000.0, 7500.0, 8000.0])
    np.testing.assert_allclose(H.mel_to_hz(H.hz_to_mel(hz)), hz, rtol=1e-12, atol=1e-9)
    assert abs(float(H.mel_to_hz(1000.0)) - 1000.0) <= 0.05
    f = H.mel_frequencies(66, H.FMIN, H.FMAX)
    assert f.shape == (66,) and abs(f[0] - 125.0) <= 1e-9 and abs(f[-1] - 7500.0) <= 1e-9 and (np.diff(f) > 0).all()


def test_filterbank_facts(mel):
    nz = mel != 0
    assert mel.shape == (64, 1025) and (mel >= 0).all()
    assert int(nz.sum()) == 1847
    per_band = nz.sum(axis=1)
    assert per_band.min() == 7 and per_band.max() == 71                   # no band is empty
    assert int(np.argmax(nz[0])) == 17 and 1024 - int(np.argmax(nz[63][::-1])) == 959
    assert (nz.sum(axis=0) <= 2).all()                                    # a bin lies inside at most two triangles
    mel_f = H.mel_frequencies(66, H.FMIN, H.FMAX)
    np.testing.assert_allclose(mel.max(axis=1), 2.0 / (mel_f[2:] - mel_f[:-2]), rtol=0.15)     # Slaney area normalisation: peak ~ 2 / width


def _band_tables(L, cfg):
    lib = L.lib()
    n = lib.mla_melspec_band_table_floats(*cfg)
    assert n > 0
    tab = np.zeros(n, dtype=np.float32)
    assert lib.mla_melspec_build_band_tables(*cfg, tab.ctypes.data_as(ctypes.c_void_p)) == 0
    return tab


def test_library_tables_match_restatement(L, mel):
    tab = _band_tables(L, CFG)
    assert np.array_equal(tab[:2048], R.hann_periodic().astype(np.float32))
    meta = tab[5120:5120 + 3 * 64].view(np.int32).reshape(64, 3)
    weights = tab[5120 + 3 * 64:]
    assert len(weights) == meta[:, 1].sum() == 1847
    assert np.array_equal(meta[:, 2], np.concatenate([[0], np.cumsum(meta[:, 1])[:-1]]))
    assert tuple(meta[0, :2]) == (17, 7) and meta[63, 0] + meta[63, 1] - 1 == 959
    dense = np.zeros((64, 1025), dtype=np.float32)
    for b, (first, bins, off) in enumerate(meta):
        assert bins >= 1 and 0 <= first and first + bins <= 1025
        dense[b, first:first + bins] = weights[off:off + bins]
    assert np.array_equal(dense != 0, mel != 0), "supports are exact"
    np.testing.assert_allclose(dense.astype(np.float64), mel, rtol=3 * 2.0 ** -24, atol=0)     # computed in double, rounded once


@pytest.mark.parametrize("n_mels", [224, 32])
def test_default_tables_are_unchanged(L, n_mels):
    lib = L.lib()
    golden = json.load(open(os.path.join(GOLDEN, "melspec_tables_sha256.json")))
    n = lib.mla_melspec_table_floats(22050.0, n_mels)
    tab = np.zeros(n, dtype=np.float32)
    assert lib.mla_melspec_build_tables(22050.0, n_mels, tab.ctypes.data_as(ctypes.c_void_p)) == 0
    assert hashlib.sha256(tab.tobytes()).hexdigest() == golden["22050_%d" % n_mels]
    # the general builder at librosa's defaults is the same table
    assert np.array_equal(_band_tables(L, (22050.0, n_mels, 0.0, 11025.0, 0)).view(np.uint32), tab.view(np.uint32))


def test_table_builder_rejects_bad_configurations(L):
    lib = L.lib()
    for cfg in ((0.0, 64, 125.0, 7500.0, 1), (16000.0, 0, 125.0, 7500.0, 1), (16000.0, 1025, 125.0, 7500.0, 1),
                (16000.0, 64, -1.0, 7500.0, 1), (16000.0, 64, 7500.0, 7500.0, 1), (16000.0, 64, 125.0, 8000.5, 1)):
        assert lib.mla_melspec_band_table_floats(*cfg) == -1, cfg
        buf = np.zeros(8, dtype=np.float32)
        assert lib.mla_melspec_build_band_tables(*cfg, buf.ctypes.data_as(ctypes.c_void_p)) == -1, cfg
    assert lib.mla_melspec_build_band_tables(*CFG, None) == -1 and b"null" in lib.mla_last_error()


def test_frame_counts_and_split_offsets(L):
    lib = L.lib()
    ds = importlib.import_module(PKG + ".dataset")
    assert (ds.SR_VGGISH, ds.SAMPLES_NUM_VGGISH_LIBROSA) == (16000, 64000)
    assert H.num_frames(64000) == 388 == lib.mla_melspec_nopad_frames(64000, 160)
    assert [lib.mla_melspec_nopad_frames(n, 160) for n in LENGTHS] == [1, 1, 2, 17, 20, 388] == [H.num_frames(n) for n in LENGTHS]
    assert lib.mla_melspec_nopad_frames(2047, 160) == -1 and lib.mla_melspec_nopad_frames(64000, 0) == -1
    step = R.split_step(388, 10, 96, True)
    assert step == 32 and 9 * step + 96 == 384 <= 388                       # the last window ends at column 384 (exclusive)
    spec = np.arange(3 * 388, dtype=np.float64).reshape(3, 388)
    fr = R.split(spec, 10, 96, True)
    assert fr.shape == (10, 3, 96) and [int(f[0, 0]) for f in fr] == [32 * t for t in range(10)] and int(fr[-1][0, -1]) + 1 == 384
    spec = np.random.default_rng(0).standard_normal((64, 388))
    assert np.array_equal(ds.split(torch.from_numpy(spec), 10, 96, 64, True).numpy(), R.split(spec, 10, 96, True))
    # 12 frames per workgroup at hop 160 (13 fit the staging buffer; cut to a multiple of the four waves): 33 runs per clip
    assert lib.mla_melspec_nopad_workspace_bytes(3, 64000, 160) == 3 * 33 * 4
    assert lib.mla_melspec_nopad_workspace_bytes(1, 2047, 160) == -1 and lib.mla_melspec_nopad_workspace_bytes(1, 64000, 0) == -1


def test_float32_baseline_stays_within_the_recorded_constants(references, mel):
    pairs = [(H.mel_power_f32(H.clip_waveform(name, n), mel=mel), ref) for (name, n), ref in references.items()]
    rel, floor = R.baseline_constants(pairs)
    print("float32 baseline on the HTK variant: rel %.3g floor %.3g" % (rel, floor))
    assert rel <= REL_BASE and floor <= FLOOR_BASE, (rel, floor)
    assert (REL, FLOOR) == (4 * REL_BASE, 4 * FLOOR_BASE)


def run_hostsim(hostsim, x, hop=H.HOP, n_mels=H.N_MELS, cfg=CFG):
    frames = H.num_frames(len(x), hop)
    out = np.full((n_mels, frames), np.nan, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    got = hostsim.hostsim_melspec_nopad_db(x.ctypes.data_as(ctypes.c_void_p), len(x), hop, cfg[0], n_mels, cfg[2], cfg[3], cfg[4], R.AMIN,
                                           out.ctypes.data_as(ctypes.c_void_p))
    assert got == frames
    return out


def test_kernel_math_on_host_matches_restatement(hostsim, references):
    worst = 0.0
    for (name, n), ref in references.items():
        D = run_hostsim(hostsim, H.clip_waveform(name, n))
        assert np.isfinite(D).all() and D.shape == ref.shape
        ok, ratio = R.power_close(R.db_to_power(D), ref, REL, FLOOR)
        worst = max(worst, ratio)
        assert ok, (name, n, ratio)
        if name == "silence":
            assert np.abs(D + 100.0).max() <= 1e-4
    print("host simulation: worst error / bound %.3f" % worst)


def test_host_simulation_run_boundaries(hostsim):
    """hop 512 leaves room for 4 frames per run (5 fit, cut to the four waves) and hop 3000 for one, with three idle waves."""
    x = H.clip_waveform("noise", 12000)
    mel32 = H.mel_filters(n_mels=32)
    for hop in (512, 3000):
        D = run_hostsim(hostsim, x, hop, 32, (float(H.SR), 32, H.FMIN, H.FMAX, 1))
        assert D.shape == (32, H.num_frames(12000, hop))
        assert R.power_close(R.db_to_power(D), H.mel_power(x, hop, mel32), REL, FLOOR)[0], hop


def test_burst_clip_sits_partly_on_the_floor(mel):
    """The GPU clip-and-gather test uses the 5 088-sample burst: between 10 % and 90 % of its elements are at max - 80 dB."""
    for n in (5088, 64000):
        D = H.melspectrogram_db(H.clip_waveform("burst", n), mel=mel)
        on_floor = float((D == D.max() - 80.0).mean())
        print("burst clip of %d samples: %.1f %% of the elements on the floor" % (n, 100 * on_floor))
        assert 0.10 <= on_floor <= 0.90, (n, on_floor)
    assert (H.melspectrogram_db(np.zeros(5088), mel=mel) == -100.0).all()


def test_argument_errors_are_reported_before_any_launch(L):
    lib = L.lib()
    vp = ctypes.c_void_p
    fake = vp(0x1000)                                # never dereferenced: every call below fails validation first
    E_ARG, E_SHAPE, E_SHORT, E_DTYPE = -1, -2, -3, -5
    cf = ctypes.c_float
    TF = 5120 + 3 * 64 + 1847

    def expect(code, rc, needle=None):
        assert rc == code, (rc, lib.mla_last_error())
        if needle:
            assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    def db(pcm=fake, clips=1, n=64000, stride=64000, hop=160, n_mels=64, amin=1e-10, tab=fake, tf=TF, out=fake, ws=fake):
        return lib.mla_melspec_nopad_db(pcm, clips, n, stride, hop, n_mels, cf(amin), tab, tf, out, ws, None)

    def bags(d=fake, ws=fake, clips=1, n=64000, hop=160, n_mels=64, top_db=80.0, n_images=10, w=96, stride=32, out=fake, dtype=0):
        return lib.mla_melspec_nopad_bags(d, ws, clips, n, hop, n_mels, cf(top_db), n_images, w, stride, out, dtype, None)

    expect(E_SHORT, db(n=2047, stride=2047), "2048")
    expect(E_SHORT, bags(n=2047), "2048")
    expect(E_ARG, db(hop=0), "hop")
    expect(E_ARG, bags(hop=0), "hop")
    expect(E_ARG, db(n_mels=0), "n_mels")
    expect(E_ARG, db(n_mels=1025), "n_mels")
    expect(E_ARG, bags(n_mels=0), "n_mels")
    expect(E_ARG, db(stride=63999), "stride")
    expect(E_ARG, db(amin=0.0), "amin")
    expect(E_ARG, db(clips=-1))
    expect(E_ARG, bags(clips=-1))
    expect(E_ARG, db(tf=5120 + 3 * 64 - 1), "table_floats")
    expect(E_ARG, db(tf=5120 + 3 * 64 + 2051), "table_floats")
    expect(E_SHAPE, db(n=(1 << 30) + 1, stride=(1 << 30) + 1), "2^30")
    for null in ("pcm", "tab", "out", "ws"):
        expect(E_ARG, db(**{null: None}), "null")
    expect(E_SHAPE, bags(stride=33), "leave")                        # 9 * 33 + 96 = 393 > 388
    expect(E_SHAPE, bags(w=389, n_images=1, stride=0), "leave")
    expect(E_SHAPE, bags(n_images=5, stride=96), "leave")            # contiguous_split: the fifth window has 4 columns
    expect(E_ARG, bags(n_images=0))
    expect(E_ARG, bags(top_db=-1.0), "top_db")
    expect(E_DTYPE, bags(dtype=2), "out_dtype")
    for null in ("d", "ws", "out"):
        expect(E_ARG, bags(**{null: None}), "null")
    assert bags(dtype=1, clips=0, d=None, ws=None, out=None) == 0
    assert db(pcm=None, clips=0, tab=None, out=None, ws=None) == 0    # no clips: nothing to do


def test_refusals_need_no_device(tmp_path):
    ds = importlib.import_module(PKG + ".dataset")
    M = importlib.import_module(PKG + ".model")
    conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    rn = M.Ensemble("repeat", conf, [2, 1], "cpu")
    pcm, rec = torch.zeros(1, 64000), [np.zeros(30000, dtype=np.int16)]
    with pytest.raises(NotImplementedError, match=r"use forward_clips\(\)"):
        rn.forward_clips_librosa(pcm)
    with pytest.raises(NotImplementedError, match=r"use forward_recordings\(\)"):
        rn.forward_recordings_librosa(rec, 16000)
    with pytest.raises(NotImplementedError, match=r"use forward_wavfiles\(\)"):
        rn.forward_wavfiles_librosa([])
    with pytest.raises(NotImplementedError, match=r"use forward_audiofiles\(\)"):
        rn.forward_audiofiles_librosa([])
    vg = M.Ensemble("repeat", dict(conf, cnn_type="vggish", just_bottlenecks=False, in_channels=1), [2, 1], "cpu")
    with pytest.raises(ValueError, match="forward_clips_librosa: overlap=False"):
        vg.forward_clips_librosa(pcm, overlap=False)
    with pytest.raises(ValueError, match="forward_recordings_librosa: overlap=False"):
        vg.forward_recordings_librosa(rec, 16000, overlap=False)
    with pytest.raises(ValueError, match="forward_wavfiles_librosa: overlap=False"):
        vg.forward_wavfiles_librosa([], overlap=False)
    with pytest.raises(ValueError, match="forward_audiofiles_librosa: overlap=False"):
        vg.forward_audiofiles_librosa([], overlap=False)
    for fn, args in ((ds.recordings_to_frames_librosa, (rec, 16000)), (ds.wavfiles_to_frames_librosa, ([],)),
                     (ds.audiofiles_to_frames_librosa, ([],))):
        with pytest.raises(ValueError, match="overlap=False"):
            fn(*args, overlap=False)
    for n in (63999, 64001, 61680):
        with pytest.raises(ValueError, match="64000"):
            ds.clips_to_frames_librosa(torch.zeros(2, n))
        with pytest.raises(ValueError, match="64000"):
            vg.forward_clips_librosa(torch.zeros(2, n))
    # the pinned refusal of create_spec now names the function that builds this path
    with pytest.raises(NotImplementedError, match="create_spec_librosa"):
        ds.create_spec(np.zeros(64000), "vggish", 16000, 64000, 96, 64, True, True)
