"""The ResNet branch's image timeline (melspec_track_* in csrc/melspec.hip, dataset.recordings_to_track_images,
Ensemble.score_image_timeline) without a GPU: the window / image / track arithmetic (mla_melspec_track_counts) against a brute-force
restatement of its definition, the descriptors' prefixes, the C ABI's argument errors, the three kernels simulated on the host
(csrc/melspec_track_hostsim.cpp: every element written once, nothing read at or behind a track's end, the powers against the float64
restatement, the images exactly the floored gather), the floor of the clip the GPU test pins the deviation with, and the Python
entries' refusals."""

import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import librosa_restated as R
from conftest import PKG, ROOT
from test_melspec_cpu import FLOOR, REL, SR

WINDOW, STEP, HOP, MELS, IMAGE_W, IMAGE_STEP, T = 88200, 7350, 98, 224, 224, 75, 10

# the ragged batch of the host simulation and of tests/test_melspec_track_gpu.py: (waveform, samples); at q = 3 four windows, one
# window with a dropped tail, one zero-filled window, and two windows the second of which ends with the recording
BATCH = (("burst", 154350), ("noise", 93200), ("chirp", 30000), ("tones", 110250))
Q = 3


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def fe(L):
    return importlib.import_module(PKG + ".frontend")


def brute_counts(n, q):
    """The definition, restated without the closed forms: windows by search for the last one that fits, images by enumeration."""
    if n >= WINDOW:
        fits = lambda j: STEP * q * j + WINDOW <= n                  # noqa: E731  window j lies inside the recording
        lo, hi = 0, 1
        while fits(hi):
            lo, hi = hi, 2 * hi
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if fits(mid) else (lo, mid)
        W = lo + 1
    else:
        W = 1
    L_ = WINDOW + STEP * q * (W - 1)
    if W <= 4096:
        kept = sum(1 for u in range(q * (W - 1) + 10) if u % q < 10)
    else:
        kept = (W - 1) * min(q, 10) + 10
    return W, kept, L_, 1 + L_ // HOP


def test_counts_match_the_definition(fe):
    table = {(1, 3): (1, 10, 88200, 901), (88199, 3): (1, 10, 88200, 901), (88200, 3): (1, 10, 88200, 901), (110249, 3): (1, 10, 88200, 901),
             (110250, 3): (2, 13, 110250, 1126), (132300, 3): (3, 16, 132300, 1351), (137300, 3): (3, 16, 132300, 1351),
             (264600, 12): (3, 30, 264600, 2701), (102900, 1): (3, 12, 102900, 1051)}
    for (n, q), want in table.items():
        assert fe.melspec_track_counts(n, q) == want == brute_counts(n, q), (n, q)
    for q in (1, 3, 10, 12):
        ns = {0, 1, WINDOW - 1, WINDOW, WINDOW + 1}
        for j in (1, 2, 3, 7):
            ns |= {WINDOW + STEP * q * j + d for d in (-1, 0, 1)}
        ns |= {2 ** 31 - 1, 2 ** 31, 2 ** 31 + STEP * q, 2 ** 40 + 12345, 2 ** 62}
        for n in sorted(ns):
            W, S, L_, C = fe.melspec_track_counts(n, q)
            assert (W, S, L_, C) == brute_counts(n, q), (n, q)
            assert C == 901 + IMAGE_STEP * q * (W - 1) and L_ <= max(n, WINDOW) and (n < WINDOW or n - L_ < STEP * q)
            assert S == (q * (W - 1) + 10 if q <= 10 else 10 * W)
            assert IMAGE_STEP * (q * (W - 1) + 9) + IMAGE_W <= C            # the last kept image lies inside the track
    ds = importlib.import_module(PKG + ".dataset")
    assert ds.image_timeline_counts(137300) == (3, 16, 132300, 1351) and ds.image_timeline_counts(264600, 12) == (3, 30, 264600, 2701)


def test_counts_entry_errors(L, fe):
    lib = L.lib()
    assert lib.mla_melspec_track_counts(100000, 0, None, None, None, None) == -1 and b"hop_images" in lib.mla_last_error()
    assert lib.mla_melspec_track_counts(-1, 3, None, None, None, None) == -1
    assert lib.mla_melspec_track_counts(100000, 3, None, None, None, None) == 0          # every output pointer may be null
    for q in (0, -2, 1.5):
        with pytest.raises(ValueError, match="hop_images must be an integer >= 1"):
            fe.melspec_track_counts(100000, q)
    with pytest.raises(ValueError):
        fe.melspec_track_counts(-1, 3)


def test_descriptor_prefixes_are_running_sums(fe):
    for lengths, q in (([n for _, n in BATCH], Q), ([264600, 5, 176400], 12), ([], 3)):
        d = fe.melspec_track_descriptors(lengths, q)
        run = col = image = 0
        assert d.host.shape == (len(lengths), 6) and d.host.dtype == np.int64
        for i, n in enumerate(lengths):
            W, S, L_, C = brute_counts(n, q)
            assert d.host[i].tolist() == [L_, C, run, MELS * col, image, q] and d.windows[i] == W
            run, col, image = run + -(-C // 16), col + C, image + S
        assert (d.runs, d.columns, d.images) == (run, col, image)
        assert d.most == max([brute_counts(n, q)[2] for n in lengths], default=0)
    d = fe.melspec_track_descriptors([n for _, n in BATCH], Q)
    assert d.windows.tolist() == [4, 1, 1, 2] and d.host[:, 0].tolist() == [154350, 88200, 88200, 110250]
    assert (d.images, d.columns, d.runs) == (19 + 10 + 10 + 13, 1576 + 901 + 901 + 1126, 99 + 57 + 57 + 71)


def test_argument_errors_are_reported_before_any_launch(L, fe):
    lib = L.lib()
    for name in ("mla_melspec_track_counts", "mla_melspec_track_db", "mla_melspec_track_images"):
        assert name in L.declared_symbols()
    vp, cf = ctypes.c_void_p, ctypes.c_float
    fake = vp(0x1000)                                    # device pointers: never dereferenced, every call below fails validation first
    E_ARG, E_SHAPE = -1, -2
    good = fe.melspec_track_descriptors([n for _, n in BATCH], Q)

    def host(desc):
        return np.ascontiguousarray(desc, dtype=np.int64)

    def db(pcm=fake, recordings=4, n_samples=good.most, row_stride=good.most, dev_desc=fake, desc=good.host, with_host=True, columns=good.columns,
           amin=1e-10, tables=fake, out=fake, ws=fake, maxima=fake):
        hd = host(desc)
        return lib.mla_melspec_track_db(pcm, recordings, n_samples, row_stride, dev_desc, hd.ctypes.data_as(vp) if with_host else None, columns,
                                        cf(amin), tables, out, ws, maxima, None)

    def images(d=fake, maxima=fake, recordings=4, dev_desc=fake, desc=good.host, with_host=True, columns=good.columns, top_db=80.0, first=0,
               count=good.images, out=fake):
        hd = host(desc)
        return lib.mla_melspec_track_images(d, maxima, recordings, dev_desc, hd.ctypes.data_as(vp) if with_host else None, columns, cf(top_db),
                                            first, count, out, None)

    def expect(code, rc, needle=None):
        assert rc == code, (rc, lib.mla_last_error())
        if needle:
            assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    def with_field(rec, field, value):
        d = good.host.copy()
        d[rec, field] = value
        return d

    for null in ("pcm", "dev_desc", "tables", "out", "ws", "maxima"):
        expect(E_ARG, db(**{null: None}), "null")
    expect(E_ARG, db(with_host=False), "null")
    expect(E_ARG, db(recordings=-1), "bad recordings")
    expect(E_ARG, db(row_stride=good.most - 1), "stride")
    expect(E_ARG, db(amin=0.0), "amin")
    expect(E_ARG, db(dev_desc=vp(0x1004)), "desc 8-byte aligned")
    expect(E_ARG, db(out=vp(0x1002)), "4-byte")
    expect(E_SHAPE, db(n_samples=good.most - 1), "recording 0: the track reads 154350 samples, the rows hold 154349")
    expect(E_ARG, db(columns=good.columns - 1), "out_db has")
    for entry in (db, images):
        expect(E_ARG, entry(desc=with_field(0, 5, 0)), "recording 0: hop_images 0")
        expect(E_ARG, entry(desc=with_field(1, 5, -3)), "recording 1: hop_images -3")
        expect(E_ARG, entry(desc=with_field(1, 0, 88200 + 7350)), "are no track")             # not a whole hop of 3 images
        expect(E_SHAPE, entry(desc=with_field(1, 0, 88199)), "recording 1: a track of 88199 samples")
        expect(E_SHAPE, entry(desc=with_field(1, 0, 88200 + 22050 * 50000)), "outside 88200 .. 2^30")
        expect(E_ARG, entry(desc=with_field(2, 1, 902)), "are no track")
        expect(E_ARG, entry(desc=with_field(1, 2, 98)), "recording 1: first_run 98")
        expect(E_ARG, entry(desc=with_field(2, 3, 0)), "db_offset 0")
        expect(E_ARG, entry(desc=with_field(3, 4, 38)), "first_image 38")
    for null in ("d", "maxima", "dev_desc", "out"):
        expect(E_ARG, images(**{null: None}), "null")
    expect(E_ARG, images(with_host=False), "null")
    expect(E_ARG, images(top_db=-1.0), "top_db")
    expect(E_ARG, images(first=-1), "bad image range")
    expect(E_ARG, images(count=-1), "bad image range")
    expect(E_ARG, images(columns=good.columns + 1), "db has")
    expect(E_ARG, images(out=vp(0x1004)), "out 16-byte aligned")
    expect(E_SHAPE, images(first=1), "images 1 .. 53 leave the 52 kept images")
    expect(E_SHAPE, images(first=good.images + 1, count=0), "leave")
    assert images(first=7, count=0, d=None, maxima=None, dev_desc=None, out=None) == 0          # an empty range: nothing to do
    assert db(recordings=0, columns=0, pcm=None, dev_desc=None, with_host=False, tables=None, out=None, ws=None, maxima=None) == 0
    assert images(recordings=0, columns=0, count=0, d=None, maxima=None, dev_desc=None, with_host=False, out=None) == 0
    expect(E_ARG, db(recordings=0, columns=3), "no recordings but 3 columns")


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("melspec_track_hostsim") / "melspec_track_hostsim.so")
    src = os.path.join(ROOT, PKG, "csrc", "melspec_track_hostsim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    lib.hostsim_melspec_track_db.restype = i64
    lib.hostsim_melspec_track_db.argtypes = [vp, i64, i64, vp, i64, ctypes.c_double, ctypes.c_float, vp, vp, vp, vp, vp]
    lib.hostsim_melspec_track_images.restype = i64
    lib.hostsim_melspec_track_images.argtypes = [vp, vp, i64, vp, ctypes.c_float, i64, i64, vp, vp]
    return lib


def batch_rows(batch, most):
    """(len(batch), most) float32 rows as the clips launch leaves them: the recording, cut at `most`, then zeros."""
    rows = np.zeros((len(batch), most), dtype=np.float32)
    for i, (name, n) in enumerate(batch):
        rows[i, :min(n, most)] = R.waveform(name, n)[:most]
    return rows


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_hostsim(hostsim, d, rows):
    Rn = rows.shape[0]
    D = np.full(MELS * d.columns, np.nan, dtype=np.float32)
    d_writes = np.zeros(MELS * d.columns, dtype=np.int32)
    partial, maxima = np.full(d.runs, np.nan, dtype=np.float32), np.full(Rn, np.nan, dtype=np.float32)
    max_read = np.zeros(Rn, dtype=np.int64)
    desc = np.ascontiguousarray(d.host)
    assert hostsim.hostsim_melspec_track_db(ptr(rows), Rn, rows.shape[1], ptr(desc), d.runs, float(SR), R.AMIN, ptr(D), ptr(d_writes),
                                            ptr(partial), ptr(maxima), ptr(max_read)) == d.runs
    return D, d_writes, maxima, max_read


def run_hostsim_images(hostsim, d, D, maxima, first, count):
    out = np.full((count, 1, MELS, IMAGE_W), np.nan, dtype=np.float32)
    writes = np.zeros(out.shape, dtype=np.int32)
    desc = np.ascontiguousarray(d.host)
    assert hostsim.hostsim_melspec_track_images(ptr(D), ptr(maxima), d.host.shape[0], ptr(desc), 80.0, first, count, ptr(out), ptr(writes)) == 49 * count
    return out, writes


def kept_images(W, q):
    return [u for u in range(q * (W - 1) + 10) if u % q < 10]


@pytest.mark.parametrize("batch,q", [(BATCH, Q), ((("burst", 154350), ("chirp", 30000)), 12)])
def test_host_simulation_of_a_ragged_batch(hostsim, fe, batch, q):
    d = fe.melspec_track_descriptors([n for _, n in batch], q)
    rows = batch_rows(batch, d.most + 500)
    for i in range(len(batch)):
        rows[i, d.host[i, 0]:] = np.nan                             # behind every track: samples there do not exist for this path
    D, d_writes, maxima, max_read = run_hostsim(hostsim, d, rows)
    assert (d_writes == 1).all() and np.isfinite(D).all() and np.isfinite(maxima).all()
    assert max_read.tolist() == (d.host[:, 0] - 1).tolist()          # the last frame is centred on the track's end: L - 1 is read, L is not
    worst = 0.0
    images, writes = run_hostsim_images(hostsim, d, D, maxima, 0, d.images)
    assert (writes == 1).all()
    for i, (name, n) in enumerate(batch):
        L_, C, _, off, first_image, _ = d.host[i].tolist()
        Dr = D[off:off + MELS * C].reshape(MELS, C)
        assert maxima[i] == Dr.max()
        track = np.zeros(L_, dtype=np.float32)
        track[:min(n, L_)] = R.waveform(name, n)[:L_]
        ok, ratio = R.power_close(R.db_to_power(Dr), R.mel_power(track, SR, MELS, HOP), REL, FLOOR)
        worst = max(worst, ratio)
        assert ok, (name, n, ratio)
        floored = np.maximum(Dr, np.float32(maxima[i]) - np.float32(80.0))
        kept = kept_images(int(d.windows[i]), q)
        assert len(kept) == (d.host[i + 1, 4] if i + 1 < len(batch) else d.images) - first_image
        for k, u in enumerate(kept):
            assert np.array_equal(images[first_image + k, 0], floored[:, IMAGE_STEP * u:IMAGE_STEP * u + IMAGE_W]), (name, u)
    print("host simulation of the tracks: worst error / bound %.3f" % worst)
    # a range of the images: the same values, every element of the range written once
    part, writes = run_hostsim_images(hostsim, d, D, maxima, 7, min(7, d.images - 7))
    assert (writes == 1).all() and np.array_equal(part, images[7:14])


def test_host_simulation_gathers_windows_that_do_not_touch(hostsim, fe):
    """q = 12 with three windows: images 10 and 11 of every hop belong to no window. On a D whose value is its column number the
    gather shows its source columns."""
    d = fe.melspec_track_descriptors([264600, 100], 12)
    assert d.windows.tolist() == [3, 1] and d.images == 40
    cols = np.concatenate([np.tile(np.arange(C, dtype=np.float32), MELS) for C in d.host[:, 1]])
    images, writes = run_hostsim_images(hostsim, d, cols, np.full(2, 80.0, dtype=np.float32), 0, d.images)        # floor 0
    assert (writes == 1).all()
    want = [12 * j + t for j in range(3) for t in range(10)] + list(range(10))
    for k, u in enumerate(want):
        assert np.array_equal(images[k, 0, 5], np.arange(IMAGE_STEP * u, IMAGE_STEP * u + IMAGE_W, dtype=np.float32)), (k, u)


def test_burst_track_sits_partly_on_the_floor():
    """tests/test_melspec_track_gpu.py pins the deviation from host crops on this track: burst, 154 350 samples, q = 3, four
    windows; the burst at sample 51 450 lies outside window 3, which starts at 66 150. Between 10 % and 90 % of the track's
    elements are at max - 80 dB, and window 3's own crop has another maximum, so its floor differs."""
    x = R.waveform("burst", 154350)
    assert brute_counts(154350, 3) == (4, 19, 154350, 1576) and 154350 // 3 == 51450 < 3 * 3 * STEP == 66150
    S = R.mel_power(x, SR, MELS, HOP)
    D = R.power_to_db(S)
    on_floor = float((D == D.max() - 80.0).mean())
    print("burst track: %.1f %% of the elements on the floor" % (100 * on_floor))
    assert 0.10 <= on_floor <= 0.90, on_floor
    crop = R.power_to_db(R.mel_power(x[66150:66150 + WINDOW], SR, MELS, HOP), top_db=None)
    assert crop.max() < D.max() - 3.0                                # the track's floor lies well above the crop's own
    # interior columns of the crop are the track's columns: the same samples in the same frames
    unclipped = R.power_to_db(S, top_db=None)
    assert np.abs(crop[:, 11:890] - unclipped[:, 675 + 11:675 + 890]).max() <= 1e-9


def test_image_timeline_entries_refuse_what_they_do_not_do():
    M = importlib.import_module(PKG + ".model")
    conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    rec = [np.zeros(100000, dtype=np.float32)]
    vg = M.Ensemble("repeat", dict(conf, cnn_type="vggish"), [2, 1], "cpu").eval()
    with pytest.raises(NotImplementedError, match=r"score_image_timeline scores .* score_timeline\(\)"):
        vg.score_image_timeline(rec, [22050])
    with pytest.raises(NotImplementedError, match=r"score_timeline_wavfiles\(\)"):
        vg.score_image_timeline_wavfiles(["nothing.wav"])
    with pytest.raises(NotImplementedError, match=r"score_timeline_audiofiles\(\)"):
        vg.score_image_timeline_audiofiles(["nothing.wav"])
    rn = M.Ensemble("repeat", conf, [2, 1], "cpu")
    assert rn.training
    for call in (lambda: rn.score_image_timeline(rec, [22050]), lambda: rn.score_image_timeline_wavfiles(["nothing.wav"]),
                 lambda: rn.score_image_timeline_audiofiles(["nothing.wav"])):
        with pytest.raises(RuntimeError, match="eval mode only"):
            call()
    rn.eval()
    with pytest.raises(ValueError, match="max_images must be >= 1"):
        rn.score_image_timeline(rec, [22050], max_images=0)
    for q in (0, 1.5):
        with pytest.raises(ValueError, match="hop_images must be an integer >= 1"):
            rn.score_image_timeline(rec, [22050], hop_images=q)
    six = M.Ensemble("repeat", conf, [2, 1], "cpu", slots=6).eval()
    with pytest.raises(ValueError, match="score_image_timeline builds the dataset's bags of 10 windows, the model takes slots = 6"):
        six.score_image_timeline(rec, [22050])
    # the existing timeline entries keep refusing the ResNet branch as they did
    with pytest.raises(NotImplementedError, match=r"score_timeline scores .* use forward_recordings\(\)"):
        rn.score_timeline(rec, [16000])


def test_python_errors_come_before_the_device_is_touched(L):
    ds = importlib.import_module(PKG + ".dataset")
    ok = np.zeros(100000, dtype=np.float32)
    for q in (0, -2, 1.5):
        with pytest.raises(ValueError, match="hop_images must be an integer >= 1"):
            ds.recordings_to_track_images([ok], 22050, hop_images=q)
    with pytest.raises(ValueError, match="2 recordings but 1 rates"):
        ds.recordings_to_track_images([ok, ok], [44100])
    with pytest.raises(TypeError, match="all int16 or all floating"):
        ds.recordings_to_track_images([ok, np.zeros(16000, dtype=np.int16)], 44100)
    with pytest.raises(ValueError, match="recording 1: Invalid sample rate"):
        ds.recordings_to_track_images([ok, ok], [22050, 0])
    with pytest.raises(ValueError, match=r"recording 1: a track of \d+ samples at 22 050 Hz is longer than 2\*\*30"):
        ds._track_lengths([100000, 2 ** 31], [22050, 22050], 3)
    with pytest.raises(ValueError, match="more than one clips launch tiles"):
        ds._track_lengths([2 ** 29] * 1200, [22050] * 1200, 3)
    n22, most = ds._track_lengths([176400, 11025, 700000], [44100, 11025, 22050], 3)
    assert n22.tolist() == [88200, 22050, 700000] and most == ds.image_timeline_counts(700000, 3)[2] == 683550
    assert ds._track_lengths([5], [22050], 3)[1] == WINDOW                 # a short recording still fills one window's row
    for fn, args in ((ds.recordings_to_track_images, ([], [])), (ds.wavfiles_to_track_images, ([],)), (ds.audiofiles_to_track_images, ([],))):
        images, first_rows, index, starts = fn(*args, hop_images=2)
        assert tuple(images.shape) == (0, 1, 224, 224) and images.dtype == torch.float32
        assert first_rows.shape == index.shape == starts.shape == (0,) and starts.dtype == np.float64
