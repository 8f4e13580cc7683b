"""WAV files of any PCM width or IEEE float -> clips on the GPU (csrc/clips.hip, clips_kernel on file bytes): the mixed batch of
tests/test_audiofiles_cpu.py against the float64 chain, the fully written output, bit-identity with the element-offset entry (the same files
decoded to float32 on the host and sent through recordings_to_clips), rows that depend on their own file only, the last 24-bit sample
of the buffer, and Ensemble.forward_audiofiles. The bound is test_clips_cpu.py's 2e-6 absolute."""

import importlib
import os

import numpy as np
import pytest
import torch

import librosa_restated as R
from conftest import PKG
from test_audiofiles_cpu import (F32, I16, I24, MULTI_I32, check_mixed_rows, make_samples, mixed_batch, write_file)
from test_clips_cpu import SAMPLES_NUMS, SR_OUT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


@pytest.fixture(scope="module")
def ds():
    return importlib.import_module(PKG + ".dataset")


@pytest.fixture(scope="module")
def batch_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("audiofiles_gpu")


@pytest.fixture(scope="module")
def rows(ds, batch_dir):
    """The mixed batch through audiofiles_to_clips, once per samples_num; the later tests compare with these rows."""
    paths = [f[0] for f in mixed_batch(batch_dir)]
    return {s: ds.audiofiles_to_clips(paths, SR_OUT, s) for s in SAMPLES_NUMS}


@pytest.mark.parametrize("samples_num", SAMPLES_NUMS)
def test_mixed_batch_matches_float64_chain(rows, batch_dir, samples_num):
    got = rows[samples_num]
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(mixed_batch(batch_dir)), samples_num)
    check_mixed_rows(got.cpu().numpy(), batch_dir, samples_num, "MI355X")


def pack(ds, paths):
    """What audiofiles_to_clips uploads: the data chunks back to back, each on a multiple of 8 bytes, in a buffer of exactly that size."""
    read = [ds.read_audiofile(p) for p in paths]
    sizes = np.array([d.shape[0] for d, _ in read], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum((sizes + 7) // 8 * 8)[:-1]]).astype(np.int64)
    packed = np.zeros(int(offsets[-1] + sizes[-1]), dtype=np.uint8)
    for (d, _), o, s in zip(read, offsets, sizes):
        packed[o:o + s] = d
    code, ch, rate, frames = zip(*(desc for _, desc in read))
    return torch.from_numpy(packed).cuda(), offsets, frames, ch, rate, code


def test_low_level_entry_writes_all_of_out(fe, ds, rows, batch_dir):
    packed, offsets, frames, ch, rate, code = pack(ds, [f[0] for f in mixed_batch(batch_dir)])
    for samples_num in SAMPLES_NUMS:
        out = torch.full((len(frames), samples_num), float("nan"), device="cuda")
        ret = fe.prepare_clips_raw(packed, offsets, frames, ch, rate, code, SR_OUT, samples_num, out=out)
        assert ret is out and not bool(torch.isnan(out).any())
        assert torch.equal(out, rows[samples_num])


def test_rows_are_bit_identical_to_the_kernel_it_extends(ds, rows, batch_dir):
    files = mixed_batch(batch_dir)
    for samples_num in SAMPLES_NUMS:
        for i, (path, code, sr_in, _, _, _) in enumerate(files):
            if i == MULTI_I32:                   # integers summed exactly and rounded once: checked against the chain only
                continue
            x, rate = ds.decode_audiofile(path)
            assert rate == sr_in
            want = ds.recordings_to_clips([x], [rate], SR_OUT, samples_num)
            assert torch.equal(rows[samples_num][i], want[0]), (path, samples_num)
            if code == I16:
                assert torch.equal(rows[samples_num][i], ds.wavfiles_to_clips([path], SR_OUT, samples_num)[0]), (path, samples_num)
    assert sum(f[1] == I16 for f in files) == 2


def test_a_row_depends_on_its_own_file_only(ds, rows, batch_dir):
    paths = [f[0] for f in mixed_batch(batch_dir)]
    for samples_num in SAMPLES_NUMS:
        for order in ([8, 7, 6, 5, 4, 3, 2, 1, 0], [4, 8, 0, 6, 2, 7, 5, 3, 1], [3, 0, 5], [0]):
            got = ds.audiofiles_to_clips([paths[i] for i in order], SR_OUT, samples_num)
            for row, i in enumerate(order):
                assert torch.equal(got[row], rows[samples_num][i]), (order, paths[i], samples_num)


@pytest.mark.parametrize("rate", [SR_OUT, 44100])
def test_24_bit_file_at_the_end_of_the_buffer(ds, tmp_path, rate):
    """The last recording of the batch is 24-bit mono with an odd number of frames, so the buffer (allocated to exactly the packed
    size) ends with its last sample's third byte. At 22 050 Hz the last sample is the last valid output itself."""
    first = write_file(tmp_path / "first.wav", I16, 32000, make_samples(I16, 777, 1, 61))
    last = write_file(tmp_path / "last.wav", I24, rate, make_samples(I24, 1501, 1, 62))
    data, desc = ds.read_audiofile(last)
    assert desc == (I24, 1, rate, 1501) and data.shape[0] == 4503 and os.path.getsize(last) % 2 == 0     # the chunk's pad byte is no sample
    x, _ = ds.decode_audiofile(last)
    for samples_num in SAMPLES_NUMS:
        got = ds.audiofiles_to_clips([first, last], SR_OUT, samples_num)
        want = ds.recordings_to_clips([x], [rate], SR_OUT, samples_num)
        assert torch.equal(got[1], want[0]), (rate, samples_num)
        if rate == SR_OUT:
            assert got[1, 1500].item() == float(x[1500]) != 0.0 and not bool(got[1, 1501:].any())


def test_forward_audiofiles(ds, tmp_path):
    M = importlib.import_module(PKG + ".model")
    W = importlib.import_module(PKG + ".weights")
    conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    ens = M.Ensemble("repeat", conf, [2, 1], torch.device("cuda"), precision="f32")
    sd = W.make_state_dict(11, W.ensemble_shapes((2, 1), True, cnn_type="resnet"))
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    ens.cuda()
    # running statistics that describe dB images, as in test_clips_gpu.py::test_forward_recordings
    calib = ds.clips_to_images(torch.from_numpy(np.stack([R.waveform("noise", 88200), R.waveform("tones", 88200)])).cuda())
    ens.train()
    with torch.no_grad():
        for _ in range(30):
            ens(calib)
    ens.eval()
    chirp = np.stack([R.waveform("chirp", 176400), R.waveform("noise", 176400)], axis=1)       # 4 s stereo at 44.1 kHz
    paths = [write_file(tmp_path / "0.wav", I24, 44100, np.round(chirp * 4000000).astype(np.int32)),
             write_file(tmp_path / "1.wav", F32, 32000, R.waveform("burst", 100000).astype(np.float32)[:, None])]
    with torch.no_grad():
        got = ens.forward_audiofiles(paths)
        assert torch.equal(got, ens.forward_clips(ds.audiofiles_to_clips(paths)))
    assert tuple(got.shape) == (2, 10) and bool(torch.isfinite(got).all())
