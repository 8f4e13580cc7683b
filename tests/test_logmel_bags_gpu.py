"""Ragged recordings -> VGGish bags on the GPU (csrc/logmel.hip, logmel_bags_kernel): bit-identity with what a user writes today (one
waveform_to_examples / wavfile_to_examples call and one re-framing per recording) in any batch order, the float64 chain for the broadband
members, the low-level entry (fully written output, bf16 = one rounding, int16 rows, unaligned rows), the launch count, WAV files and
the model entries. The bound, 1e-4 absolute, and why it is applied to broadband rows only: tests/test_logmel_bags_cpu.py.

The batch holds the ten 16 kHz lengths of the CPU test and five resampled recordings, 15 in all: every count 0..4 occurs on both sides."""

import importlib
import wave

import numpy as np
import pytest
import torch

from conftest import PKG
from oracle import dataset_frames as ods
from oracle import resample as oresample
from test_audiofiles_cpu import F32, I24, write_file
from test_logmel_bags_cpu import LENGTHS, ROW, TOL, noise, oracle_frames, rows_and_counts

pytestmark = pytest.mark.gpu

# (rate, channels, frames): n_res = 64 000 (4 examples), 32 000 (2), 15 600 by the library's length (1: the 15 599 / 15 600 edge),
# 48 000 (3), 8 000 (0)
RESAMPLED = ((44100, 2, 176400), (8000, 1, 16000), (48000, 1, 46800), (22050, 1, 66150), (192000, 2, 96000))
CASES = tuple((16000, 1, n) for n in LENGTHS) + RESAMPLED
RATES = [c[0] for c in CASES]
BROADBAND = tuple(range(len(LENGTHS))) + tuple(len(LENGTHS) + i for i in (0, 2, 3, 4))      # all but the upsampled 8 kHz member
ORDERS = ([14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0], [7, 12, 0, 10, 3, 14, 5, 1, 11, 9, 2, 13, 6, 8, 4])


def make_recording(index, int16):
    """Seeded samples of case `index`: the CPU test's noise for the float 16 kHz members, else uniform in [-0.5, 0.5] float32 or int16
    in +-16 000; (n,) for mono, else (n, channels)."""
    _, ch, n = CASES[index]
    if index < len(LENGTHS) and not int16:
        return noise(index, n)
    rng = np.random.default_rng(9000 + 2 * index + int(int16))
    x = rng.integers(-16000, 16001, size=(n, ch)).astype(np.int16) if int16 else rng.uniform(-0.5, 0.5, size=(n, ch)).astype(np.float32)
    return x[:, 0].copy() if ch == 1 else x


def write_wav(path, pcm, rate):
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1])
        wf.setsampwidth(2)
        wf.setframerate(rate)
        wf.writeframes(pcm.tobytes())
    return str(path)


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


@pytest.fixture(scope="module")
def ds():
    return importlib.import_module(PKG + ".dataset")


@pytest.fixture(scope="module")
def recs():
    return {int16: [make_recording(i, int16) for i in range(len(CASES))] for int16 in (False, True)}


@pytest.fixture(scope="module")
def batch(ds, recs):
    """Batch R through recordings_to_frames, once per (int16, overlap); the later tests compare with these rows."""
    return {(int16, overlap): ds.recordings_to_frames(recs[int16], RATES, overlap) for int16 in (False, True) for overlap in (True, False)}


def expected_counts(L):
    lib = L.lib()
    n_res = [n if r == 16000 else int(lib.mla_resample_length(n, float(r), 16000.0)) for r, _, n in CASES]
    return n_res, [max(0, (1 + (n - 400) // 160) // 96) for n in n_res]


def test_counts_follow_the_library(batch):
    L = importlib.import_module(PKG + "._lib")
    n_res, counts = expected_counts(L)
    assert n_res[len(LENGTHS) + 2] in (15599, 15600)
    assert sorted(set(counts[:len(LENGTHS)])) == [0, 1, 2, 3, 4] and sorted(set(counts[len(LENGTHS):])) == [0, 1, 2, 3, 4]
    for key, got in batch.items():
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(CASES), 10 if key[1] else 4, 1, 64, 96)
        spec = torch.cat([got[:, t, 0] for t in ((0, 3, 6, 9) if key[1] else (0, 1, 2, 3))], dim=2)      # (B, 64, 384)
        filled = (spec != 0).reshape(len(CASES), 64, 4, 96).any(dim=3).any(dim=1).sum(dim=1).cpu().tolist()
        assert filled == counts, (key, filled, counts)


def today(ds, x, rate, overlap, tmp_path):
    """What a user writes today for one recording: waveform_to_examples (wavfile_to_examples on a 16-bit file for int16 samples), the
    create_spec-style (64, 384) spectrogram, split."""
    VI = importlib.import_module(PKG + ".torchvggish.vggish_input")
    if x.dtype == np.int16:
        ex = VI.wavfile_to_examples(write_wav(tmp_path / "one.wav", x, rate))
    else:
        ex = VI.waveform_to_examples(x, rate)
    ex = ex.detach().reshape(-1, 96, 64)
    return ds.split(ds._frames(ex, 1, ex.shape[0], 1, 384, 0)[0, 0], 10, 96, 64, overlap)


@pytest.mark.parametrize("int16", [False, True])
def test_rows_are_bit_identical_to_the_per_recording_calls(ds, recs, batch, tmp_path, int16):
    r = recs[int16]
    for overlap in (True, False):
        want = [today(ds, r[i], RATES[i], overlap, tmp_path) for i in range(len(CASES))]
        got = batch[int16, overlap]
        for i in range(len(CASES)):
            assert torch.equal(got[i, :, 0], want[i]), (CASES[i], overlap)
        # other orders and B = 1: a row depends on its own recording only
        for order in list(ORDERS) + [[i] for i in range(len(CASES))]:
            got = ds.recordings_to_frames([r[i] for i in order], [RATES[i] for i in order], overlap)
            for row, i in enumerate(order):
                assert torch.equal(got[row, :, 0], want[i]), (order, CASES[i], overlap)


def mono_f32(x):
    x2 = x.reshape(x.shape[0], -1).astype(np.float64)
    return (x2.sum(axis=1) / x2.shape[1] * (1.0 / 32768.0 if x.dtype == np.int16 else 1.0)).astype(np.float32)


_chain = {}


def chain_frames(recs, index, int16, overlap):
    """float64 frames of one broadband member: the mono mix rounded to float32 as the kernel's is, oracle/resample.py, then
    split(create_spec_native(.)); computed once and never modified."""
    if index < len(LENGTHS) and not int16:
        return oracle_frames(index, overlap)
    key = (index, int16)
    if key not in _chain:
        m = mono_f32(recs[int16][index]).astype(np.float64)
        y = m if RATES[index] == 16000 else oresample.resample(m, RATES[index], 16000)
        spec = ods.create_spec_native(y)
        spec.setflags(write=False)
        _chain[key] = spec
    return np.asarray(ods.split(_chain[key], 10, 96, 64, overlap))


@pytest.mark.parametrize("int16", [False, True])
def test_broadband_rows_match_float64_chain(recs, batch, int16):
    worst = 0.0
    for overlap in (True, False):
        got = batch[int16, overlap].cpu().numpy()[:, :, 0]
        for i in BROADBAND:
            ref = chain_frames(recs, i, int16, overlap)
            assert ref.shape == got[i].shape
            assert np.array_equal(got[i] == 0.0, ref == 0.0), (CASES[i], overlap, "zero pattern")
            err = float(np.abs(got[i].astype(np.float64) - ref).max())
            worst = max(worst, err)
            print("%s %s overlap=%s: |d| %.3g" % (CASES[i], "int16" if int16 else "float32", overlap, err))
            assert err <= TOL, (CASES[i], overlap, err)
    print("MI355X, %s: worst |d| %.3g (bound %.3g)" % ("int16" if int16 else "float32", worst, TOL))


def test_low_level_entry(fe, ds):
    rows, counts = rows_and_counts()
    B = rows.shape[0]
    pcm = torch.from_numpy(rows).cuda()
    for n_frames, stride in ((10, 32), (4, 96)):
        out = torch.full((B, n_frames, 1, 64, 96), float("nan"), device="cuda")
        ret = fe.logmel_bags(pcm, counts, n_frames, stride, out=out)
        assert ret is out and not bool(torch.isnan(out).any())
        # the two kernels it replaces, on the rows cut to what their examples read
        for c in range(B):
            ex = fe.waveforms_to_examples(pcm[c:c + 1, :15600 + 15360 * (int(counts[c]) - 1)]) if counts[c] else torch.empty((0, 96, 64), device="cuda")
            assert torch.equal(out[c, :, 0], ds._frames(ex, 1, int(counts[c]), n_frames, 96, stride)[0]), (LENGTHS[c], n_frames)
        # counts as a device tensor: read back first, the same launch
        assert torch.equal(fe.logmel_bags(pcm, torch.from_numpy(counts).cuda(), n_frames, stride), out)
        # bf16 is one rounding of the float32 value
        half = torch.full((B, n_frames, 1, 64, 96), float("nan"), device="cuda", dtype=torch.bfloat16)
        assert fe.logmel_bags(pcm, counts, n_frames, stride, torch.bfloat16, out=half) is half
        assert torch.equal(half.view(torch.int16), out.to(torch.bfloat16).view(torch.int16))
        # rows that are not 8-byte aligned take the kernel's scalar loads: the same bits
        wide = torch.full((B, ROW + 1), float("nan"), device="cuda")
        wide[:, 1:] = pcm
        assert wide[:, 1:].data_ptr() % 8 == 4
        assert torch.equal(fe.logmel_bags(wide[:, 1:], counts, n_frames, stride), out)
        # samples past what a row's examples read are never touched
        poisoned = pcm.clone()
        for c in range(B):
            poisoned[c, (15600 + 15360 * (int(counts[c]) - 1) if counts[c] else 0):] = float("nan")
        assert torch.equal(fe.logmel_bags(poisoned, counts, n_frames, stride), out)
    # int16 rows at 16 kHz equal the float32 rows of the same samples / 32768
    rng = np.random.default_rng(77)
    pcm16 = rng.integers(-16000, 16001, size=(5, ROW)).astype(np.int16)
    c5 = np.array([4, 0, 2, 1, 3], dtype=np.int32)
    as_float = torch.from_numpy(pcm16.astype(np.float32) / np.float32(32768.0)).cuda()
    for n_frames, stride in ((10, 32), (4, 96)):
        want = fe.logmel_bags(as_float, c5, n_frames, stride)
        assert torch.equal(fe.logmel_bags(torch.from_numpy(pcm16).cuda(), c5, n_frames, stride), want)
        odd = torch.zeros((5, ROW + 1), dtype=torch.int16, device="cuda")
        odd[:, 1:] = torch.from_numpy(pcm16).cuda()
        assert odd[:, 1:].data_ptr() % 4 == 2
        assert torch.equal(fe.logmel_bags(odd[:, 1:], c5, n_frames, stride), want)
        assert torch.equal(fe.logmel_bags(torch.from_numpy(pcm16).cuda(), c5, n_frames, stride, torch.bfloat16).view(torch.int16),
                           want.to(torch.bfloat16).view(torch.int16))


def test_two_launches(ds, recs, batch):
    ops = importlib.import_module(PKG + ".ops")
    saved = ops.profile
    try:
        ops.profile = []
        got = ds.recordings_to_frames(recs[False], RATES)
        assert [p[0] for p in ops.profile] == ["clips_prepare", "logmel_bags"]
        ops.profile = []
        one = ds.recordings_to_frames(recs[False][10:11], RATES[10:11])
        assert [p[0] for p in ops.profile] == ["clips_prepare", "logmel_bags"]
    finally:
        ops.profile = saved
    assert torch.equal(got, batch[False, True]) and torch.equal(one[0], batch[False, True][10])


def test_files(ds, recs, batch, tmp_path):
    picks = [10, 2, 13, 0, 14, 7, 12]
    paths = [write_wav(tmp_path / ("%d.wav" % i), recs[True][i], RATES[i]) for i in picks]
    for overlap in (True, False):
        got = ds.wavfiles_to_frames(paths, overlap)
        assert torch.equal(got, ds.recordings_to_frames([recs[True][i] for i in picks], [RATES[i] for i in picks], overlap))
        assert torch.equal(got, batch[True, overlap][picks])
        assert torch.equal(ds.audiofiles_to_frames(paths, overlap), got)
        assert torch.equal(ds.audiofiles_to_frames(paths, overlap, torch.bfloat16).view(torch.int16), got.to(torch.bfloat16).view(torch.int16))
    # a 24-bit and a float32 copy of one recording (stereo, 44.1 kHz): decoded at full precision in the clips launch
    x = recs[False][10]
    others = [write_file(tmp_path / "a24.wav", I24, 44100, np.round(x.astype(np.float64) * 8000000).astype(np.int32)),
              write_file(tmp_path / "f32.wav", F32, 44100, x), paths[1]]
    got = ds.audiofiles_to_frames(others)
    for row, path in enumerate(others[:2]):
        decoded, rate = ds.decode_audiofile(path)
        assert rate == 44100 and decoded.dtype == np.float32 and decoded.shape == x.shape
        assert torch.equal(got[row], ds.recordings_to_frames([decoded], [rate])[0]), path
    assert torch.equal(got[1], batch[False, True][10]) and torch.equal(got[2], batch[True, True][2])
    with pytest.raises(AssertionError, match="Bad sample type: 3"):
        ds.wavfiles_to_frames([others[0]])


def test_model_entries(ds, recs, tmp_path):
    M = importlib.import_module(PKG + ".model")
    W = importlib.import_module(PKG + ".weights")
    conf = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=1)
    ens = M.Ensemble("repeat", conf, [2, 1], torch.device("cuda"))
    sd = W.make_state_dict(6, W.ensemble_shapes((2, 1), False))
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    ens.cuda().eval()
    half_second = np.random.default_rng(5).integers(-16000, 16001, size=8000).astype(np.int16)
    picks = [10, 13, 5]
    r, rates = [recs[True][i] for i in picks] + [half_second], [RATES[i] for i in picks] + [16000]
    paths = [write_wav(tmp_path / ("%d.wav" % i), x, rate) for i, (x, rate) in enumerate(zip(r, rates))]
    with torch.no_grad():
        frames = ds.recordings_to_frames(r, rates)
        assert not bool(frames[3].any()) and bool(frames[:3].any())
        got = ens.set_precision("f32").forward_recordings_native(r, rates)
        assert torch.equal(got, ens(frames))
        assert tuple(got.shape) == (4, 10) and bool(torch.isfinite(got).all())
        assert torch.equal(ens.forward_wavfiles_native(paths), got) and torch.equal(ens.forward_audiofiles_native(paths), got)
        ens.set_precision("bf16")
        half = ds.recordings_to_frames(r, rates, out_dtype=torch.bfloat16)
        assert half.dtype == torch.bfloat16 and torch.equal(half.view(torch.int16), frames.to(torch.bfloat16).view(torch.int16))
        want = ens.mla(ens.cnn(half.view(-1, 96, 64)).reshape(-1, 10, ens.emb_input_size))
        got16 = ens.forward_recordings_native(r, rates)
        assert torch.equal(got16, want) and bool(torch.isfinite(got16).all())
        assert torch.equal(ens.forward_wavfiles_native(paths), got16) and torch.equal(ens.forward_audiofiles_native(paths), got16)
    with pytest.raises(NotImplementedError, match=r"use forward_recordings_native\(\)"):
        ens.forward_recordings(r, rates)
