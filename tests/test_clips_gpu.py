"""Recordings -> clips on the GPU (csrc/clips.hip): the mixed batch of tests/test_clips_cpu.py's cases against the float64 chain, the
fully written output, bit-identity with the per-recording calls it replaces (frontend.as_device_mono + frontend.resample, cut and
zero-filled) in any batch order, the workload's shape once, WAV files, and Ensemble.forward_recordings. The bound is test_clips_cpu.py's
2e-6 absolute."""

import importlib
import wave

import numpy as np
import pytest
import torch

import librosa_restated as R
from conftest import PKG
from test_clips_cpu import ALL_CASES, CASES, SAMPLES_NUMS, SR_OUT, TOL, check_rows, cut_and_fill, make_recording, pack, resampled_f64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


@pytest.fixture(scope="module")
def ds():
    return importlib.import_module(PKG + ".dataset")


RATES = [c[0] for c in ALL_CASES]


@pytest.mark.parametrize("int16", [False, True])
@pytest.mark.parametrize("samples_num", SAMPLES_NUMS)
def test_mixed_batch_matches_float64_chain(ds, samples_num, int16):
    recs = [make_recording(i, int16) for i in range(len(ALL_CASES))]
    got = ds.recordings_to_clips(recs, RATES, SR_OUT, samples_num)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(ALL_CASES), samples_num)
    check_rows(got.cpu().numpy(), int16, samples_num, "MI355X")


def test_low_level_entry_writes_all_of_out(fe):
    recs = [make_recording(i, False) for i in range(len(ALL_CASES))]
    frames = np.array([x.shape[0] for x in recs], dtype=np.int64)
    channels = np.array([c[1] for c in ALL_CASES], dtype=np.int32)
    sizes = frames * channels
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    packed = torch.from_numpy(np.concatenate([x.reshape(-1) for x in recs])).cuda()
    for samples_num in SAMPLES_NUMS:
        out = torch.full((len(recs), samples_num), float("nan"), device="cuda")
        # descriptors as device tensors here, host arrays in recordings_to_clips: the same launch
        ret = fe.prepare_clips(packed, torch.from_numpy(offsets).cuda(), torch.from_numpy(frames).cuda(), torch.from_numpy(channels).cuda(),
                               torch.tensor(RATES, dtype=torch.float64).cuda(), SR_OUT, samples_num, out=out)
        assert ret is out and not bool(torch.isnan(out).any())
        check_rows(out.cpu().numpy(), False, samples_num, "MI355X, prepare_clips")


@pytest.mark.parametrize("int16", [False, True])
def test_element_and_byte_offsets_give_the_same_rows(fe, int16):
    """One kernel serves both entries: the same packed buffer through prepare_clips (element offsets) and through prepare_clips_raw
    (viewed as bytes, offsets x sample size, one format code for all) gives the same bits."""
    L = importlib.import_module(PKG + "._lib")
    recs = [make_recording(i, int16) for i in range(len(ALL_CASES))]
    host, offsets, frames, channels = pack(recs)
    packed = torch.from_numpy(host).cuda()
    typed = fe.prepare_clips(packed, offsets, frames, channels, RATES, SR_OUT, 2000)
    formats = np.full(len(recs), L.I16 if int16 else L.F32, dtype=np.int32)
    raw = fe.prepare_clips_raw(packed.view(torch.uint8), offsets * host.itemsize, frames, channels, RATES, formats, SR_OUT, 2000)
    assert bool(torch.isfinite(typed).all())
    assert torch.equal(typed.view(torch.int32), raw.view(torch.int32))


def per_recording(fe, x, sr_in, samples_num):
    """What the caller had to write before: one mono mix, one resampling launch, a slice and a copy into zeros, per recording."""
    if x.dtype == np.int16:
        x = (x.astype(np.float32) / np.float32(32768.0))          # exact: a power of two
    y = fe.resample(fe.as_device_mono(x, pcm16=False), sr_in, SR_OUT)
    row = torch.zeros(samples_num, dtype=torch.float32, device="cuda")
    k = min(y.shape[0], samples_num)
    row[:k] = y[:k]
    return row


@pytest.mark.parametrize("int16", [False, True])
def test_rows_are_bit_identical_to_the_per_recording_calls(fe, ds, int16):
    n = len(CASES)
    recs = [make_recording(i, int16) for i in range(n)]
    for samples_num in SAMPLES_NUMS:
        want = [per_recording(fe, recs[i], CASES[i][0], samples_num) for i in range(n)]
        got = ds.recordings_to_clips(recs, RATES[:n], SR_OUT, samples_num)
        for i in range(n):
            assert torch.equal(got[i], want[i]), (CASES[i], samples_num)
        # another order and other batch sizes: a row depends on its own recording only
        for order in ([5, 0, 7, 3], [6], [2, 4, 1, 6, 0, 3, 7, 5]):
            got = ds.recordings_to_clips([recs[i] for i in order], [RATES[i] for i in order], SR_OUT, samples_num)
            for row, i in enumerate(order):
                assert torch.equal(got[row], want[i]), (order, CASES[i], samples_num)


def test_workload_shape(ds):
    rng = np.random.default_rng(7)
    stereo = rng.integers(-16000, 16001, size=(176400, 2)).astype(np.int16)         # 4 s at 44.1 kHz
    mono48 = rng.uniform(-0.5, 0.5, size=153600).astype(np.float32)                # 3.2 s at 48 kHz
    long22 = rng.integers(-16000, 16001, size=110250).astype(np.int16)             # 5 s at 22.05 kHz
    a = ds.recordings_to_clips([stereo, long22], [44100, 22050])
    b = ds.recordings_to_clips([mono48], 48000)
    assert tuple(a.shape) == (2, 88200) and tuple(b.shape) == (1, 88200)
    clips = torch.cat([a[:1], b, a[1:]]).cpu().numpy()
    assert clips.shape == (3, 88200)
    for row, x, sr_in in ((0, stereo, 44100), (1, mono48, 48000)):
        err = float(np.abs(clips[row] - cut_and_fill(resampled_f64(x, sr_in), 88200)).max())
        print("workload row %d: |d| %.3g (bound %.3g)" % (row, err, TOL))
        assert err <= TOL, (row, err)
    assert np.array_equal(clips[2], long22[:88200].astype(np.float32) / np.float32(32768.0))
    assert int(153600 * 22050 / 48000) == 70560 and not clips[1, 70560:].any() and clips[1, 70559] != 0.0


def write_wav(path, pcm, rate, width=2):
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1])
        wf.setsampwidth(width)
        wf.setframerate(rate)
        wf.writeframes(pcm.tobytes())


def test_wav_files(ds, tmp_path):
    rng = np.random.default_rng(8)
    mono = rng.integers(-16000, 16001, size=3000).astype(np.int16)
    stereo = rng.integers(-16000, 16001, size=(6001, 2)).astype(np.int16)
    write_wav(tmp_path / "mono.wav", mono, 22050)
    write_wav(tmp_path / "stereo.wav", stereo, 44100)
    paths = [tmp_path / "mono.wav", tmp_path / "stereo.wav"]
    for samples_num in SAMPLES_NUMS:
        got = ds.wavfiles_to_clips(paths, samples_num=samples_num)
        assert torch.equal(got, ds.recordings_to_clips([mono, stereo], [22050, 44100], samples_num=samples_num))
    pcm, rate = ds.read_wav16(str(paths[1]))
    assert rate == 44100 and np.array_equal(pcm, stereo)
    write_wav(tmp_path / "eight.wav", (mono >> 8).astype(np.int8).view(np.uint8), 22050, width=1)
    with pytest.raises(AssertionError, match="Bad sample type: 1"):
        ds.wavfiles_to_clips([tmp_path / "eight.wav"])


def test_forward_recordings(ds, tmp_path):
    M = importlib.import_module(PKG + ".model")
    W = importlib.import_module(PKG + ".weights")
    conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    ens = M.Ensemble("repeat", conf, [2, 1], torch.device("cuda"), precision="f32")
    sd = W.make_state_dict(11, W.ensemble_shapes((2, 1), True, cnn_type="resnet"))
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    ens.cuda()
    # running statistics that describe dB images, as in test_melspec_gpu.py::test_forward_clips
    calib = ds.clips_to_images(torch.from_numpy(np.stack([R.waveform("noise", 88200), R.waveform("tones", 88200)])).cuda())
    ens.train()
    with torch.no_grad():
        for _ in range(30):
            ens(calib)
    ens.eval()
    chirp = np.stack([R.waveform("chirp", 176400), R.waveform("noise", 176400)], axis=1)       # 4 s stereo at 44.1 kHz
    recs, rates = [(chirp * 16000).astype(np.int16), (R.waveform("burst", 100000) * 16000).astype(np.int16)], [44100, 32000]
    with torch.no_grad():
        got = ens.forward_recordings(recs, rates)
        clips = ds.recordings_to_clips(recs, rates)
        assert torch.equal(got, ens.forward_clips(clips))
        assert torch.equal(got, ens(ds.clips_to_images(clips)))
    assert tuple(got.shape) == (2, 10) and bool(torch.isfinite(got).all())
    for i, (x, r) in enumerate(zip(recs, rates)):
        write_wav(tmp_path / ("%d.wav" % i), x, r)
    with torch.no_grad():
        assert torch.equal(ens.forward_wavfiles([tmp_path / "0.wav", tmp_path / "1.wav"]), got)
