"""The ResNet branch's mel-dB front-end on the GPU (csrc/melspec.hip) against the float64 restatement of the librosa calls
(tests/librosa_restated.py): small shapes where the indexing can go wrong, batch invariance, the workload's two shapes, the
clip-and-gather kernel bit for bit, and Ensemble.forward_clips. The tolerance is test_melspec_cpu.py's (REL, FLOOR): four times
the float32 baseline, in the power domain ("mel-dB front-end tolerance")."""

import importlib

import numpy as np
import pytest
import torch

import librosa_restated as R
from conftest import PKG
from test_melspec_cpu import FLOOR, REL, SHAPES, SR

pytestmark = pytest.mark.gpu

N_CLIP = 88200


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


@pytest.fixture(scope="module")
def ds():
    return importlib.import_module(PKG + ".dataset")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def assert_power_close(D, ref_power, what):
    S = R.db_to_power(D)
    ok, ratio = R.power_close(S, ref_power, REL, FLOOR)
    print("%s: worst error / bound %.3f" % (what, ratio))
    assert ok, (what, ratio)
    return S


@pytest.mark.parametrize("n,hop,n_mels", SHAPES)
def test_small_shapes_match_restatement(fe, n, hop, n_mels):
    waves = np.stack([R.waveform(name, n) for name in R.WAVEFORMS])
    D = fe.melspectrogram_db(dev(waves), SR, n_mels, hop, top_db=None).cpu().numpy()
    frames = R.num_frames(n, hop)
    assert D.shape == (len(R.WAVEFORMS), n_mels, frames) and np.isfinite(D).all()
    assert frames == {(1025, 98): 11, (4096, 128): 33, (5000, 98): 52, (5000, 39): 129}[(n, hop)]
    for i, name in enumerate(R.WAVEFORMS):
        ref = R.mel_power(waves[i], SR, n_mels, hop)
        S = assert_power_close(D[i], ref, "%s n=%d hop=%d" % (name, n, hop))
        for sl in (slice(0, 11), slice(-11, None)):              # the frames that read reflected samples pass on their own
            assert R.power_close(S[:, sl], ref[:, sl], REL, FLOOR)[0], (name, sl)
        if name == "silence":
            assert np.abs(D[i] + 100.0).max() <= 1e-4 and np.unique(D[i]).size == 1


def test_run_boundaries(fe):
    """hop 512 leaves room for 5 frames per workgroup instead of 16, hop 3000 for one."""
    x = R.waveform("noise", 12000)
    for hop in (512, 3000):
        D = fe.melspectrogram_db(dev(x[None]), SR, 32, hop, top_db=None).cpu().numpy()[0]
        assert_power_close(D, R.mel_power(x, SR, 32, hop), "noise hop=%d" % hop)


@pytest.mark.parametrize("n,hop,n_mels,samples_num,x_size,overlap",
                         [(5000, 98, 224, 88200, 224, True), (5000, 39, 224, 88200, 224, False), (4096, 128, 32, 4096, 8, True)])
def test_create_spec_is_the_clipped_spectrogram(fe, ds, n, hop, n_mels, samples_num, x_size, overlap):
    x = R.waveform("burst", n)
    spec = ds.create_spec(x.astype(np.float64), "resnet", SR, samples_num, x_size, n_mels, False, overlap)   # use_librosa is forced on
    assert tuple(spec.shape) == (n_mels, R.num_frames(n, hop)) and spec.is_cuda
    D = fe.melspectrogram_db(dev(x[None]), SR, n_mels, hop, top_db=None)[0]
    assert torch.equal(spec, torch.maximum(D, D.max() - 80.0))
    assert torch.equal(spec, ds.create_spec(x, "resnet", SR, samples_num, x_size, n_mels, True, overlap))
    ref = R.melspectrogram_db(x, SR, n_mels, hop)
    assert_power_close(spec.cpu().numpy(), R.db_to_power(ref), "create_spec n=%d hop=%d" % (n, hop))


def test_batch_invariance_and_row_stride(fe):
    n = 5000
    waves = np.stack([R.waveform(name, n) for name in ("noise", "chirp", "burst")])
    alone = [fe.melspectrogram_db(dev(waves[i:i + 1]), SR, 224, 98, top_db=None)[0] for i in range(3)]
    clipped = [fe.melspectrogram_db(dev(waves[i:i + 1]), SR, 224, 98)[0] for i in range(3)]
    for B in (1, 2, 3):
        D = fe.melspectrogram_db(dev(waves[:B]), SR, 224, 98, top_db=None)
        C = fe.melspectrogram_db(dev(waves[:B]), SR, 224, 98)
        for i in range(B):
            assert torch.equal(D[i], alone[i]) and torch.equal(C[i], clipped[i]), (B, i)
    # the last clip first: the position in the batch does not matter either
    D = fe.melspectrogram_db(dev(waves[::-1]), SR, 224, 98, top_db=None)
    assert all(torch.equal(D[2 - i], alone[i]) for i in range(3))
    wide = torch.full((3, n + 1000), float("nan"), device="cuda")
    wide[:, :n] = dev(waves)
    D = fe.melspectrogram_db(wide[:, :n], SR, 224, 98, top_db=None)
    assert wide[:, :n].stride(0) == n + 1000 and all(torch.equal(D[i], alone[i]) for i in range(3))


def test_short_clip_raises(fe, ds):
    with pytest.raises(ValueError, match="1025"):
        fe.melspectrogram_db(torch.zeros(1, 1024, device="cuda"), SR, 224, 98)
    with pytest.raises(ValueError):
        ds.clips_to_images(torch.zeros(2, 88199, device="cuda"))


def test_workload_overlapping_images(ds):
    names = ("noise", "chirp", "burst")
    waves = np.stack([R.waveform(name, N_CLIP) for name in names])
    images = ds.clips_to_images(dev(waves), overlap=True)
    assert tuple(images.shape) == (3, 10, 1, 224, 224) and images.dtype == torch.float32
    for i, name in enumerate(names):
        spec = ds.create_spec(waves[i], "resnet", SR, N_CLIP, 224, 224, True, True)
        assert tuple(spec.shape) == (224, 901)
        assert torch.equal(images[i, :, 0], ds.split(spec, 10, 224, 224, True)), name
        ref = R.split(R.melspectrogram_db(waves[i], SR, 224, 98), 10, 224, True)
        got = images[i, :, 0].cpu().numpy()
        for t in range(10):
            ok, ratio = R.power_close(R.db_to_power(got[t]), R.db_to_power(ref[t]), REL, FLOOR)
            assert ok, (name, t, ratio)


def test_workload_contiguous_images(ds):
    x = R.waveform("tones", N_CLIP)
    images = ds.clips_to_images(dev(x[None]), overlap=False)
    assert tuple(images.shape) == (1, 10, 1, 224, 224)
    spec = ds.create_spec(x, "resnet", SR, N_CLIP, 224, 224, True, False)
    assert tuple(spec.shape) == (224, 2262)
    assert torch.equal(images[0, :, 0], ds.split(spec, 10, 224, 224, False))
    full = R.melspectrogram_db(x, SR, 224, 39)
    assert_power_close(spec.cpu().numpy(), R.db_to_power(full), "tones hop=39, 2262 frames")
    ref = R.split(full, 10, 224, False)
    got = images[0, :, 0].cpu().numpy()
    assert all(R.power_close(R.db_to_power(got[t]), R.db_to_power(ref[t]), REL, FLOOR)[0] for t in range(10))


def test_clip_and_gather_are_exact(fe):
    """From the GPU's own unclipped D the images are max(D, D.max() - 80) gathered at the split offsets, bit for bit; the burst clip
    has the floor active on part of it (test_melspec_cpu.py asserts 10..90 % on the restatement)."""
    waves = np.stack([R.waveform("burst", N_CLIP), np.zeros(N_CLIP, dtype=np.float32), R.waveform("noise", N_CLIP)])
    D, ws = fe.melspec_db_unclipped(dev(waves), SR, 224, 98)
    images = fe.melspec_images(D, ws, N_CLIP, 98, 80.0, 10, 224, 75)
    assert tuple(D.shape) == (3, 224, 901) and tuple(images.shape) == (3, 10, 1, 224, 224)
    for c in range(3):
        assert ws.reshape(3, -1)[c].max() == D[c].max()
        clipped = torch.maximum(D[c], D[c].max() - 80.0)
        for t in range(10):
            assert torch.equal(images[c, t, 0], clipped[:, 75 * t:75 * t + 224]), (c, t)
    on_floor = float((images[0] == D[0].max() - 80.0).float().mean())
    assert 0.10 <= on_floor <= 0.90, on_floor
    silent = images[1]
    assert torch.unique(silent).numel() == 1 and abs(float(silent.flatten()[0]) + 100.0) <= 1e-4
    assert not bool((images[2] == D[2].max() - 80.0).any())        # white noise never reaches the floor
    # another window over the same D: one image per clip, the whole spectrogram, top_db 20
    whole = fe.melspec_images(D, ws, N_CLIP, 98, 20.0, 1, 901, 0)
    assert all(torch.equal(whole[c, 0, 0], torch.maximum(D[c], D[c].max() - 20.0)) for c in range(3))


@pytest.mark.parametrize("input_conf", ["repeat", "single"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_forward_clips(ds, input_conf, precision):
    M = importlib.import_module(PKG + ".model")
    W = importlib.import_module(PKG + ".weights")
    conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    ens = M.Ensemble(input_conf, conf, [2, 1], torch.device("cuda"), precision=precision)
    sd = W.make_state_dict(11, W.ensemble_shapes((2, 1), True, cnn_type="resnet"))
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    ens.cuda()
    # The seeded running statistics describe unit-scale inputs; dB images are a hundred times larger, and with such statistics the
    # eval-mode head's attention underflows to 0 / 0 = NaN exactly as the reference's would. A trained model's statistics describe its
    # data: thirty train-mode passes over two OTHER clips move them there (momentum 0.1: 96 % of the way).
    calib = ds.clips_to_images(dev(np.stack([R.waveform("noise", N_CLIP), R.waveform("tones", N_CLIP)])))
    ens.train()
    with torch.no_grad():
        for _ in range(30):
            ens(calib)
    ens.eval()
    pcm = dev(np.stack([R.waveform("chirp", N_CLIP), R.waveform("burst", N_CLIP)]))
    with torch.no_grad():
        got = ens.forward_clips(pcm)
        ref = ens(ds.clips_to_images(pcm))
    assert tuple(got.shape) == (2, 10) and bool(torch.isfinite(got).all())
    assert torch.equal(got, ref)
