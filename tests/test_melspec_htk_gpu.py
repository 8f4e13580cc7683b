"""The VGGish branch's librosa path on the GPU (csrc/melspec.hip: melspec_nopad_db_kernel, melspec_images_kernel) against the
float64 restatement (tests/librosa_htk_restated.py): the lengths where the framing and the runs can go wrong, batch invariance, the
clip-and-gather kernel bit for bit in float32 and bfloat16, the workload, recordings and files, and the model entries. The
tolerance is test_melspec_cpu.py's (REL, FLOOR), four times the float32 baseline in the power domain."""

import importlib
import wave

import numpy as np
import pytest
import torch

import librosa_htk_restated as H
import librosa_restated as R
from conftest import PKG
from test_melspec_cpu import FLOOR, REL

pytestmark = pytest.mark.gpu

SMALL = (2048, 2207, 2208, 4608, 5088)
KW = dict(center=False, htk=True, fmin=H.FMIN, fmax=H.FMAX)


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


@pytest.fixture(scope="module")
def ds():
    return importlib.import_module(PKG + ".dataset")


@pytest.fixture(scope="module")
def mel():
    return H.mel_filters()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def assert_power_close(D, ref_power, what):
    ok, ratio = R.power_close(R.db_to_power(D), ref_power, REL, FLOOR)
    print("%s: worst error / bound %.3f" % (what, ratio))
    assert ok, (what, ratio)


@pytest.mark.parametrize("n", SMALL)
def test_small_lengths_match_restatement(fe, mel, n):
    waves = np.stack([H.clip_waveform(name, n) for name in R.WAVEFORMS])
    D = fe.melspectrogram_db(dev(waves), H.SR, 64, 160, top_db=None, **KW).cpu().numpy()
    frames = {2048: 1, 2207: 1, 2208: 2, 4608: 17, 5088: 20}[n]
    assert D.shape == (len(R.WAVEFORMS), 64, frames) and np.isfinite(D).all()
    for i, name in enumerate(R.WAVEFORMS):
        assert_power_close(D[i], H.mel_power(waves[i], mel=mel), "%s n=%d" % (name, n))
        if name == "silence":
            assert np.abs(D[i] + 100.0).max() <= 1e-4 and np.unique(D[i]).size == 1


def test_run_boundaries(fe):
    """hop 512 leaves room for 4 frames per workgroup (one round of the four waves), hop 3000 for one (three idle waves)."""
    x = H.clip_waveform("noise", 12000)
    mel32 = H.mel_filters(n_mels=32)
    for hop in (512, 3000):
        D = fe.melspectrogram_db(dev(x[None]), H.SR, 32, hop, top_db=None, **KW).cpu().numpy()[0]
        assert D.shape == (32, H.num_frames(12000, hop))
        assert_power_close(D, H.mel_power(x, hop, mel32), "noise hop=%d" % hop)


def test_batch_invariance_and_row_stride(fe):
    n = 5088
    waves = np.stack([H.clip_waveform(name, n) for name in ("noise", "chirp", "burst")])
    alone = [fe.melspectrogram_db(dev(waves[i:i + 1]), H.SR, 64, 160, top_db=None, **KW)[0] for i in range(3)]
    clipped = [fe.melspectrogram_db(dev(waves[i:i + 1]), H.SR, 64, 160, **KW)[0] for i in range(3)]
    for B in (1, 2, 3):
        D = fe.melspectrogram_db(dev(waves[:B]), H.SR, 64, 160, top_db=None, **KW)
        C = fe.melspectrogram_db(dev(waves[:B]), H.SR, 64, 160, **KW)
        for i in range(B):
            assert torch.equal(D[i], alone[i]) and torch.equal(C[i], clipped[i]), (B, i)
    D = fe.melspectrogram_db(dev(waves[::-1]), H.SR, 64, 160, top_db=None, **KW)
    assert all(torch.equal(D[2 - i], alone[i]) for i in range(3))
    wide = torch.full((3, n + 1000), float("nan"), device="cuda")
    wide[:, :n] = dev(waves)
    D = fe.melspectrogram_db(wide[:, :n], H.SR, 64, 160, top_db=None, **KW)
    assert wide[:, :n].stride(0) == n + 1000 and all(torch.equal(D[i], alone[i]) for i in range(3))


def test_short_clip_raises(fe, ds):
    with pytest.raises(ValueError, match="2048"):
        fe.melspectrogram_db(torch.zeros(1, 2047, device="cuda"), H.SR, 64, 160, **KW)
    with pytest.raises(ValueError, match="2048"):
        ds.create_spec_librosa(np.zeros(2047))
    with pytest.raises(ValueError, match="64000"):
        ds.clips_to_frames_librosa(torch.zeros(2, 63999, device="cuda"))


def test_clip_and_gather_are_exact(fe):
    """From the GPU's own unclipped D: three windows of width 8 at stride 6 over the 20 frames of 5 088 samples equal
    max(D, D.max() - 80) at their offsets bit for bit, and the bf16 output is the float32 output rounded to nearest even."""
    n = 5088
    waves = np.stack([H.clip_waveform("burst", n), np.zeros(n, dtype=np.float32), H.clip_waveform("noise", n)])
    D, ws = fe.melspec_db_unclipped_librosa(dev(waves), H.SR, 64, 160, H.FMIN, H.FMAX, True)
    images = fe.melspec_bags(D, ws, n, 160, 80.0, 3, 8, 6)
    assert tuple(D.shape) == (3, 64, 20) and tuple(images.shape) == (3, 3, 1, 64, 8) and images.dtype == torch.float32
    for c in range(3):
        assert ws.reshape(3, -1)[c].max() == D[c].max()
        clipped = torch.maximum(D[c], D[c].max() - 80.0)
        for t in range(3):
            assert torch.equal(images[c, t, 0], clipped[:, 6 * t:6 * t + 8]), (c, t)
    whole = fe.melspec_bags(D, ws, n, 160, 80.0, 1, 20, 0)
    on_floor = float((whole[0] == D[0].max() - 80.0).float().mean())
    print("burst clip: %.1f %% of the elements on the floor" % (100 * on_floor))
    assert 0.10 <= on_floor <= 0.90, on_floor
    silent = images[1]
    assert torch.unique(silent).numel() == 1 and abs(float(silent.flatten()[0]) + 100.0) <= 1e-4
    assert not bool((images[2] == D[2].max() - 80.0).any())        # white noise never reaches the floor
    half = fe.melspec_bags(D, ws, n, 160, 80.0, 3, 8, 6, torch.bfloat16)
    assert half.dtype == torch.bfloat16 and torch.equal(half.view(torch.int16), images.to(torch.bfloat16).view(torch.int16))
    half = fe.melspec_bags(D, ws, n, 160, 80.0, 1, 20, 0, torch.bfloat16)
    assert torch.equal(half.view(torch.int16), whole.to(torch.bfloat16).view(torch.int16))


@pytest.fixture(scope="module")
def workload(ds):
    names = ("noise", "chirp", "burst")
    waves = np.stack([H.clip_waveform(name, H.N_CLIP) for name in names])
    return names, waves, ds.clips_to_frames_librosa(dev(waves))


def test_workload(ds, mel, workload):
    names, waves, bags = workload
    assert tuple(bags.shape) == (3, 10, 1, 64, 96) and bags.dtype == torch.float32
    for i, name in enumerate(names):
        spec = ds.create_spec_librosa(waves[i])
        assert tuple(spec.shape) == (64, 388) and spec.is_cuda
        assert torch.equal(bags[i, :, 0], ds.split(spec, 10, 96, 64, True)), name
        ref = R.split(H.melspectrogram_db(waves[i], mel=mel), 10, 96, True)
        got = bags[i, :, 0].cpu().numpy()
        for t in range(10):
            ok, ratio = R.power_close(R.db_to_power(got[t]), R.db_to_power(ref[t]), REL, FLOOR)
            assert ok, (name, t, ratio)
    half = ds.clips_to_frames_librosa(dev(waves), torch.bfloat16)
    assert torch.equal(half.view(torch.int16), bags.to(torch.bfloat16).view(torch.int16))


def write_wav(path, pcm, rate):
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(rate)
        wf.writeframes(pcm.tobytes())
    return str(path)


@pytest.fixture(scope="module")
def recordings():
    rng = np.random.default_rng(77)
    return [rng.integers(-16000, 16001, size=n).astype(np.int16) for n in (30000, 70000)]


def fitted(recordings):
    rows = np.zeros((len(recordings), H.N_CLIP), dtype=np.float32)
    for i, x in enumerate(recordings):
        m = min(len(x), H.N_CLIP)
        rows[i, :m] = x[:m].astype(np.float32) / np.float32(32768.0)
    return rows


def test_recordings_and_files(ds, recordings, tmp_path):
    ops = importlib.import_module(PKG + ".ops")
    want = ds.clips_to_frames_librosa(dev(fitted(recordings)))
    saved = ops.profile
    try:
        ops.profile = []
        got = ds.recordings_to_frames_librosa(recordings, 16000)
        assert [p[0] for p in ops.profile] == ["clips_prepare", "melspec_nopad_db", "melspec_nopad_bags"]      # three launches
    finally:
        ops.profile = saved
    assert tuple(got.shape) == (2, 10, 1, 64, 96) and torch.equal(got, want)
    paths = [write_wav(tmp_path / ("%d.wav" % i), x, 16000) for i, x in enumerate(recordings)]
    assert torch.equal(ds.wavfiles_to_frames_librosa(paths), want)
    assert torch.equal(ds.audiofiles_to_frames_librosa(paths), want)
    assert torch.equal(ds.audiofiles_to_frames_librosa(paths, out_dtype=torch.bfloat16).view(torch.int16),
                       want.to(torch.bfloat16).view(torch.int16))
    assert tuple(ds.recordings_to_frames_librosa([], []).shape) == (0, 10, 1, 64, 96)


def test_model_entries(ds, recordings, tmp_path):
    M = importlib.import_module(PKG + ".model")
    W = importlib.import_module(PKG + ".weights")
    conf = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=1)
    ens = M.Ensemble("repeat", conf, [2, 1], torch.device("cuda"))
    sd = W.make_state_dict(6, W.ensemble_shapes((2, 1), False))
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    ens.cuda()
    # The seeded running statistics describe unit-scale inputs; dB bags are far from that, and with such statistics the eval-mode
    # head's attention can underflow to 0 / 0 = NaN exactly as the reference's would (tests/test_melspec_gpu.py::test_forward_clips).
    # Thirty train-mode passes over two OTHER clips move the statistics to the data (momentum 0.1: 96 % of the way).
    calib = ds.clips_to_frames_librosa(dev(np.stack([H.clip_waveform("noise", H.N_CLIP), H.clip_waveform("tones", H.N_CLIP)])))
    ens.train()
    with torch.no_grad():
        for _ in range(30):
            ens(calib)
    ens.eval()
    pcm = dev(np.stack([H.clip_waveform("chirp", H.N_CLIP), H.clip_waveform("burst", H.N_CLIP)]))
    paths = [write_wav(tmp_path / ("%d.wav" % i), x, 16000) for i, x in enumerate(recordings)]
    with torch.no_grad():
        ens.set_precision("f32")
        got = ens.forward_clips_librosa(pcm)
        assert tuple(got.shape) == (2, 10) and bool(torch.isfinite(got).all())
        assert torch.equal(got, ens(ds.clips_to_frames_librosa(pcm)))
        rec = ens.forward_recordings_librosa(recordings, 16000)
        assert torch.equal(rec, ens(ds.recordings_to_frames_librosa(recordings, 16000))) and bool(torch.isfinite(rec).all())
        assert torch.equal(ens.forward_wavfiles_librosa(paths), rec) and torch.equal(ens.forward_audiofiles_librosa(paths), rec)
        ens.set_precision("bf16")
        half = ds.clips_to_frames_librosa(pcm, torch.bfloat16)
        got16 = ens.forward_clips_librosa(pcm)
        assert bool(torch.isfinite(got16).all()) and torch.equal(got16, ens(half))
        rec16 = ens.forward_recordings_librosa(recordings, 16000)
        assert torch.equal(rec16, ens(ds.recordings_to_frames_librosa(recordings, 16000, out_dtype=torch.bfloat16)))
        assert torch.equal(ens.forward_wavfiles_librosa(paths), rec16) and torch.equal(ens.forward_audiofiles_librosa(paths), rec16)
    with pytest.raises(NotImplementedError, match="forward_waveforms"):
        ens.forward_clips(pcm)
