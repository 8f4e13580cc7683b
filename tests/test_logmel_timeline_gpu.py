"""Recordings of any length scored over time on the GPU: dataset.recordings_to_slots (the clips launch, then logmel_timeline_kernel),
ops.gather_bags and Ensemble.score_timeline.

What pins the values is bit identity with the code that already exists: ten consecutive rows from a window's first row equal the bag
frontend.logmel_bags gives for that window's crop of the resampled recording. This holds because a crop starts a multiple of 32 columns
(5 120 samples) into the recording and a work item is 8 columns of adjacent frame pairs: column c of the recording is column c - 32 q j of
the crop, it falls into the same item position and the same frame pair on both routes, reads the same samples and runs the same pair_step.

A batch is all int16 or all floating (dataset._checked_recordings), so the issue's batch comes as two: FLOAT holds the six 16 kHz noise
recordings, a short one with two examples, and the 44.1 kHz stereo recording as float32; INT16 holds that recording as int16 beside an
int16 16 kHz one."""

import importlib
import wave

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

WINDOW, HOP = 61680, 5120
QS = (1, 3, 10, 12)
LENGTHS = (61679, 61680, 61680 + HOP * 3 - 1, 61680 + HOP * 3, 128000, 8000, 40000)
STEREO = (44100, 2, 308700)                        # 7 s; 112 000 samples at 16 kHz


def noise(index, n):
    return np.random.default_rng(9100 + index).uniform(-0.5, 0.5, size=n).astype(np.float32)


def make_batches():
    rng = np.random.default_rng(9200)
    stereo16 = rng.integers(-16000, 16001, size=(STEREO[2], STEREO[1])).astype(np.int16)
    mono16 = rng.integers(-16000, 16001, size=100000).astype(np.int16)
    flt = [noise(i, n) for i, n in enumerate(LENGTHS)] + [(stereo16.astype(np.float32) / np.float32(32768.0))]
    return {"float": (flt, [16000] * len(LENGTHS) + [STEREO[0]]), "int16": ([stereo16, mono16], [STEREO[0], 16000])}


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


@pytest.fixture(scope="module")
def ds():
    return importlib.import_module(PKG + ".dataset")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def batches():
    return make_batches()


@pytest.fixture(scope="module")
def whole(ds, batches):
    """Every recording at 16 kHz, whole, as the clips launch gives it alone: {(batch, index): (1, n16) device tensor}. Computed once."""
    out = {}
    for name, (recs, rates) in batches.items():
        n16, _ = ds._timeline_lengths([x.shape[0] for x in recs], rates, 1)
        for i, (x, r) in enumerate(zip(recs, rates)):
            out[name, i] = ds.recordings_to_clips([x], [r], sr=16000, samples_num=int(n16[i]))
    return out


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def window_bags(ds, fe, batches, whole, name, i, q, dtype):
    """The bags existing code gives for the windows of recording i: (W, 10, 64, 96)."""
    clip = whole[name, i]
    n = clip.shape[1]
    if n < WINDOW:
        recs, rates = batches[name]
        return ds.recordings_to_frames([recs[i]], [rates[i]], out_dtype=dtype).view(1, 10, 64, 96)
    W = 1 + (n - WINDOW) // (HOP * q)
    four = np.array([4], dtype=np.int32)
    return torch.cat([fe.logmel_bags(clip[:, HOP * q * j:HOP * q * j + WINDOW], four, out_dtype=dtype).view(1, 10, 64, 96) for j in range(W)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("q", QS)
def test_windows_are_bit_identical_to_the_bags_of_their_crops(ds, fe, batches, whole, q, dtype):
    for name, (recs, rates) in batches.items():
        slots, first_rows, index, starts = ds.recordings_to_slots(recs, rates, hop_slots=q, out_dtype=dtype)
        assert slots.dtype == dtype and slots.dim() == 3 and tuple(slots.shape[1:]) == (64, 96)
        counts = [ds.timeline_counts(whole[name, i].shape[1], q) for i in range(len(recs))]
        assert slots.shape[0] == sum(c[1] for c in counts) and first_rows.shape[0] == sum(c[0] for c in counts)
        assert index.tolist() == [i for i, c in enumerate(counts) for _ in range(c[0])]
        assert np.allclose(starts, [0.32 * q * j for c in counts for j in range(c[0])], rtol=0, atol=1e-12) and starts.dtype == np.float64
        w = 0
        for i in range(len(recs)):
            want = window_bags(ds, fe, batches, whole, name, i, q, dtype)
            assert want.shape[0] == counts[i][0]
            for j in range(want.shape[0]):
                got = slots[first_rows[w]:first_rows[w] + 10]
                assert torch.equal(bits(got), bits(want[j])), (name, i, q, j)
                w += 1
        assert w == first_rows.shape[0]


def test_rows_depend_on_their_own_recording_only(ds, batches):
    recs, rates = batches["float"]
    for q in (3, 12):
        slots, first_rows, index, _ = ds.recordings_to_slots(recs, rates, hop_slots=q)
        n_slots = [ds.timeline_counts(ds._timeline_lengths([x.shape[0]], [r], q)[0][0], q)[1] for x, r in zip(recs, rates)]
        first = np.concatenate([[0], np.cumsum(n_slots)])
        order = [4, 7, 0, 5, 2, 6, 1, 3]
        mixed = ds.recordings_to_slots([recs[i] for i in order], [rates[i] for i in order], hop_slots=q)[0]
        at = 0
        for i in order:
            assert torch.equal(mixed[at:at + n_slots[i]], slots[first[i]:first[i + 1]]), (q, i)
            at += n_slots[i]
        for i in range(len(recs)):
            alone = ds.recordings_to_slots([recs[i]], [rates[i]], hop_slots=q)[0]
            assert torch.equal(alone, slots[first[i]:first[i + 1]]), (q, i)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_out_is_overwritten_and_nothing_behind_samples_read_is_read(ds, fe, batches, dtype):
    recs, rates = batches["float"]
    for q in (1, 3, 12):
        n16, most = ds._timeline_lengths([x.shape[0] for x in recs], rates, q)
        clips = ds.recordings_to_clips(recs, rates, sr=16000, samples_num=most)
        want, first_rows, _ = fe.logmel_timeline(clips, n16, q, dtype)
        out = torch.full_like(want, float("nan"))
        got, fr2, _ = fe.logmel_timeline(clips, n16, q, dtype, out=out)
        assert got is out and not bool(torch.isnan(out).any()) and torch.equal(bits(out), bits(want)) and np.array_equal(fr2, first_rows)
        poisoned = clips.clone()
        for i, n in enumerate(n16):
            poisoned[i, ds.timeline_counts(int(n), q)[2]:] = float("nan")
        assert bool(torch.isnan(poisoned).any())
        assert torch.equal(bits(fe.logmel_timeline(poisoned, n16, q, dtype)[0]), bits(want)), q
    # int16 rows, and rows at an odd element offset (the scalar sample loads), give the bits of the same samples as float32
    n16, most = ds._timeline_lengths([x.shape[0] for x in recs[:5]], rates[:5], 3)
    pcm16 = np.stack([np.pad((x * 32768.0).astype(np.int16), (0, most))[:most] for x in recs[:5]])
    as_float = torch.from_numpy(pcm16.astype(np.float32) / np.float32(32768.0)).cuda()
    want = fe.logmel_timeline(as_float, n16, 3, dtype)[0]
    assert torch.equal(bits(fe.logmel_timeline(torch.from_numpy(pcm16).cuda(), n16, 3, dtype)[0]), bits(want))
    odd = torch.zeros((5, most + 3), dtype=torch.float32, device="cuda")
    odd[:, 1:most + 1] = as_float
    assert torch.equal(bits(fe.logmel_timeline(odd[:, 1:most + 1], n16, 3, dtype)[0]), bits(want))


def test_two_launches(ds, ops, batches):
    recs, rates = batches["float"]
    saved = ops.profile
    try:
        ops.profile = []
        ds.recordings_to_slots(recs, rates)
        assert [p[0] for p in ops.profile] == ["clips_prepare", "logmel_timeline"]
        ops.profile = []
        ds.recordings_to_slots(recs[4:5], rates[4:5], hop_slots=12, out_dtype=torch.bfloat16)
        assert [p[0] for p in ops.profile] == ["clips_prepare", "logmel_timeline"]
    finally:
        ops.profile = saved


@pytest.mark.parametrize("W", [1, 5])
def test_gather_bags(ops, W):
    T = 10
    g = torch.Generator().manual_seed(3)
    first = np.array([7, 0, 3, 21, 3][:W], dtype=np.int64)
    idx = (torch.from_numpy(first)[:, None] + torch.arange(T)).reshape(-1).cuda()
    wide = torch.randn((31, 128), generator=g).cuda()
    assert torch.equal(ops.gather_bags(wide, first, T), wide[idx])
    assert torch.equal(ops.gather_bags(wide, torch.from_numpy(first).cuda(), T), wide[idx])          # a device tensor is read back
    base = torch.randn((31, 7), generator=g).cuda()
    narrow = base[:, 1:]                                          # M = 6, ld = 7, rows 4 bytes off 16-byte alignment
    assert narrow.shape[1] == 6 and narrow.stride(0) == 7 and narrow.data_ptr() % 16 == 4
    assert torch.equal(ops.gather_bags(narrow, first, T), narrow[idx])
    strided = torch.randn((31, 132), generator=g).cuda()[:, :128]        # M = 128, ld = 132: 16-byte accesses with a row pitch
    assert torch.equal(ops.gather_bags(strided, first, T), strided[idx])
    assert tuple(ops.gather_bags(wide, np.zeros(0, dtype=np.int64), T).shape) == (0, 128)
    with pytest.raises(RuntimeError, match="leave emb"):
        ops.gather_bags(wide, np.array([22], dtype=np.int64), T)


def write_wav(path, pcm, rate):
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1])
        wf.setsampwidth(2)
        wf.setframerate(rate)
        wf.writeframes(pcm.tobytes())
    return str(path)


@pytest.fixture(scope="module")
def ens():
    M = importlib.import_module(PKG + ".model")
    W = importlib.import_module(PKG + ".weights")
    conf = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=1)
    model = M.Ensemble("repeat", conf, [2, 1], torch.device("cuda"))
    sd = W.make_state_dict(6, W.ensemble_shapes((2, 1), False))
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return model.cuda().eval()


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_model_entries(ds, batches, ens, tmp_path, precision):
    """score_timeline against the route a user had before it: crops on the host, one bag per crop, ens(recordings_to_frames(crops)).
    The CNN's result for an example does not depend on the batch it sits in -- measured on the code before this entry existed: 40
    examples through ens.cnn as one batch, in chunks of 16 and one at a time give the same bits in f32, bf16x3 and bf16 (DESIGN.md
    section 4) -- so the scores are equal bit for bit, across the routes and across max_slots."""
    ens.set_precision(precision)
    recs, rates = batches["float"]
    q = 3
    with torch.no_grad():
        scores, index, starts = ens.score_timeline(recs, rates, hop_slots=q)
        n16 = ds._timeline_lengths([x.shape[0] for x in recs], rates, q)[0]
        windows = [ds.timeline_counts(int(n), q)[0] for n in n16]
        assert windows == [1, 1, 1, 2, 5, 1, 1, 4]
        assert tuple(scores.shape) == (sum(windows), 10) and scores.dtype == torch.float32 and bool(torch.isfinite(scores).all())
        assert index.dtype == np.int64 and index.tolist() == [i for i, w in enumerate(windows) for _ in range(w)]
        assert starts.dtype == np.float64 and np.allclose(starts, [0.96 * j for w in windows for j in range(w)], rtol=0, atol=1e-12)
        chunked = ens.score_timeline(recs, rates, hop_slots=q, max_slots=16)[0]
        print("%s: max_slots 16 against one chunk, max |d score| %.3g" % (precision, float((chunked - scores).abs().max())))
        # the 16 kHz recordings: a host crop holds the very samples of the window (the resampled one is pinned by the slots' bits)
        crops, rows = [], []
        w = 0
        for i, x in enumerate(recs):
            for j in range(windows[i]):
                if rates[i] == 16000:
                    crops.append(x[HOP * q * j:HOP * q * j + WINDOW] if x.shape[0] >= WINDOW else x)
                    rows.append(w)
                w += 1
        per_crop = ens.forward_recordings_native(crops, 16000)
        print("%s: timeline against per-crop bags, max |d score| %.3g" % (precision, float((scores[rows] - per_crop).abs().max())))
        if precision == "f32":
            assert torch.equal(ens(ds.recordings_to_frames(crops, 16000)), per_crop)
        assert torch.equal(scores[rows], per_crop)
        assert torch.equal(chunked, scores)
        # files: 16-bit WAV through both readers equals the arrays
        recs16, rates16 = batches["int16"]
        paths = [write_wav(tmp_path / ("%d.wav" % i), x, r) for i, (x, r) in enumerate(zip(recs16, rates16))]
        want, want_index, want_starts = ens.score_timeline(recs16, rates16, hop_slots=2)
        for got in (ens.score_timeline_wavfiles(paths, hop_slots=2), ens.score_timeline_audiofiles(paths, hop_slots=2, max_slots=16)):
            assert torch.equal(got[0], want) and np.array_equal(got[1], want_index) and np.array_equal(got[2], want_starts)
        assert want.shape[0] == sum(ds.timeline_counts(n, 2)[0] for n in (112000, 100000))
    ens.set_precision("f32")
