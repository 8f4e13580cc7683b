"""Recordings of any length -> the distinct slots of their windows (csrc/logmel.hip logmel_timeline_kernel, csrc/logmel_timeline_core.h)
without a GPU: the window / slot arithmetic (mla_timeline_counts) against a brute-force restatement of its definition; the kernel's work
items simulated on the host (csrc/logmel_timeline_hostsim.cpp: logmel_core.h's phases, the shared item / slot / offset arithmetic)
against the float64 chain oracle.dataset_frames.split(create_spec_native(crop)) of every window's crop; the C ABI's argument errors; the
Python refusals that come before the device is touched.

The bound, 1e-4 absolute on broadband input (uniform noise of amplitude 0.5), is the one of tests/test_logmel_bags_cpu.py, for its
reasons."""

import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from oracle import dataset_frames as ods

WINDOW, HOP, FIRST, EXAMPLE = 61680, 5120, 15600, 15360
TOL = 1e-4
QS = (1, 2, 3, 7, 10, 11, 12, 25)
# short recordings with 0, 0, 1, 2, 3 examples, long ones of one window, of several, and with a trailing stretch that is dropped
BATCH = (240, 15599, 15600, 30960, 61679, 61680, 61680 + 3 * HOP - 1, 61680 + 12 * HOP + 17, 128000)


def noise(index, n):
    """Seeded uniform noise of amplitude 0.5 at 16 kHz, float32."""
    return np.random.default_rng(9000 + index).uniform(-0.5, 0.5, size=n).astype(np.float32)


def brute(n, q):
    """The issue's definition, restated slot by slot: (windows, kept slots in order of u, samples read, window j -> its ten rows)."""
    assert n >= 240 and q >= 1
    if n >= WINDOW:
        W = 0
        while HOP * q * W + WINDOW <= n:          # window W's crop [5120 q W, 5120 q W + 61680) fits
            W += 1
        read = HOP * q * (W - 1) + WINDOW
    else:
        W = 1
        examples = 0
        while FIRST + EXAMPLE * examples <= n:
            examples += 1
        read = FIRST + EXAMPLE * (examples - 1) if examples else 0
    kept = sorted({q * j + t for j in range(W) for t in range(10)})
    assert all(u % q < 10 for u in kept)
    rows = [[kept.index(q * j + t) for t in range(10)] for j in range(W)] if W < 200 else None
    return W, kept, read, rows


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("logmel_timeline_hostsim") / "logmel_timeline_hostsim.so")
    src = os.path.join(ROOT, PKG, "csrc", "logmel_timeline_hostsim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.hostsim_logmel_timeline.argtypes = [vp, i64, i64, i64, vp, i64, vp, vp, vp, i64, vp]
    lib.hostsim_timeline_counts.argtypes = [i64, i64] + [ctypes.POINTER(i64)] * 6
    return lib


def lengths_of(q):
    return (240, 15599, 15600, 61679, 61680, 61680 + HOP * q - 1, 61680 + HOP * q, 61680 + HOP * q * 3 + 17)


@pytest.mark.parametrize("q", QS)
def test_timeline_counts_against_the_definition(L, hostsim, q):
    fe = importlib.import_module(PKG + ".frontend")
    ds = importlib.import_module(PKG + ".dataset")
    for n in lengths_of(q):
        W, kept, read, rows = brute(n, q)
        assert fe.timeline_counts(n, q) == (W, len(kept), read), (n, q)
        assert ds.timeline_counts(n, q) == (W, len(kept), read)
        # the closed forms the issue states
        assert len(kept) == (q * (W - 1) + 10 if q <= 10 else 10 * W)
        step = q if q <= 10 else 10
        assert rows == [list(range(step * j, step * j + 10)) for j in range(W)]
        # the header's arithmetic as the kernel compiles it (host build), and the descriptors Python derives from the library's counts
        v = [ctypes.c_int64() for _ in range(6)]
        assert hostsim.hostsim_timeline_counts(n, q, *[ctypes.byref(x) for x in v]) == 0
        w_, s_, cols, spec, items, rd = [x.value for x in v]
        assert (w_, s_, rd) == (W, len(kept), read)
        assert cols == 32 * q * (W - 1) + 384 and spec == (cols if n >= WINDOW else max(read - 240, 0) // 160)
        desc, windows, total, most = fe.timeline_descriptors([n, n], q)
        assert desc.tolist() == [[0, cols, spec, 0, q], [len(kept), cols, spec, items, q]]
        assert windows.tolist() == [W, W] and total == 2 * len(kept) and most == read


def test_timeline_counts_beyond_32_bits(L):
    """37 hours at 16 kHz: n, 160 * columns and 5 120 q (W - 1) all pass 2**31."""
    fe = importlib.import_module(PKG + ".frontend")
    n = 2 ** 31 + 100000                      # the trailing stretch that is dropped is shorter than 5 120 * 12 samples
    assert n // 160 * 160 > 2 ** 31
    for q in (1, 3, 12):
        W = 1 + (n - WINDOW) // (HOP * q)
        slots = q * (W - 1) + 10 if q <= 10 else 10 * W
        assert fe.timeline_counts(n, q) == (W, slots, WINDOW + HOP * q * (W - 1))
        assert WINDOW + HOP * q * (W - 1) > 2 ** 31
    # a very long hop: one window however large q is
    assert fe.timeline_counts(10 ** 9, 10 ** 6) == (1, 10, WINDOW)


def test_timeline_counts_errors(L):
    fe = importlib.import_module(PKG + ".frontend")
    lib = L.lib()
    with pytest.raises(ValueError, match="negative dimensions"):
        fe.timeline_counts(239, 3)
    for q in (0, -1, 2.5):
        with pytest.raises(ValueError, match="hop_slots"):
            fe.timeline_counts(100000, q)
    assert lib.mla_timeline_counts(100000, 0, None, None, None) == -1 and b"hop_slots" in lib.mla_last_error()
    assert lib.mla_timeline_counts(-1, 3, None, None, None) == -1
    assert lib.mla_timeline_counts(239, 3, None, None, None) == L.E_SHORT
    assert lib.mla_timeline_counts(100000, 3, None, None, None) == 0              # every output pointer may be null


def run_hostsim(hostsim, fe, cases, q):
    """The recordings BATCH[i], i in `cases`, through the host simulation -> (out, desc, windows, computed, max_read). Whatever lies
    past a recording's counted samples is NaN in its row: it must never be read."""
    lengths = [BATCH[i] for i in cases]
    desc, windows, total, most = fe.timeline_descriptors(lengths, q)
    R = len(lengths)
    rows = np.full((R, most), np.nan, dtype=np.float32)
    for r, i in enumerate(cases):
        k = fe.timeline_counts(BATCH[i], q)[2]
        rows[r, :k] = noise(i, BATCH[i])[:k]
    out = np.full((total, 64, 96), np.nan, dtype=np.float32)
    writes = np.zeros(out.shape, dtype=np.int32)
    pitch = int(desc[:, 1].max())
    computed = np.zeros((R, pitch), dtype=np.int32)
    max_read = np.zeros(R, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = hostsim.hostsim_logmel_timeline(p(rows), R, most, most, p(desc), total, p(out), p(writes), p(computed), pitch, p(max_read))
    assert rc == 0, rc
    assert (writes == 1).all(), "every element of out is written exactly once"
    assert not np.isnan(out).any()
    return out, desc, windows, computed, max_read


@pytest.mark.parametrize("q", (1, 3, 10, 12))
def test_hostsim_writes_every_element_once_from_the_right_place(L, hostsim, q):
    fe = importlib.import_module(PKG + ".frontend")
    out, desc, windows, computed, max_read = run_hostsim(hostsim, fe, range(len(BATCH)), q)
    step = q if q <= 10 else 10
    worst = 0.0
    for i, n in enumerate(BATCH):
        W, kept, read, _ = brute(n, q)
        assert windows[i] == W
        # a column is computed once iff it lies in a kept slot and has a spectrum; the highest sample read is samples_read - 1
        want = np.zeros(computed.shape[1], dtype=np.int32)
        for u in kept:
            want[32 * u:32 * u + 96] = 1
        want[int(desc[i, 2]):] = 0
        assert np.array_equal(computed[i], want), (n, q)
        assert max_read[i] == read - 1, (n, q, max_read[i], read)
        wave = noise(i, n).astype(np.float64)
        for j in range(W):
            crop = wave[HOP * q * j:HOP * q * j + WINDOW] if n >= WINDOW else wave
            ref = np.asarray(ods.split(ods.create_spec_native(crop), 10, 96, 64, True))          # (10, 64, 96)
            first = int(desc[i, 0]) + step * j
            got = out[first:first + 10]
            assert np.array_equal(got == 0.0, ref == 0.0), (n, q, j, "zero pattern")
            worst = max(worst, float(np.abs(got.astype(np.float64) - ref).max()))
    print("host simulation, hop_slots %d: worst |d| %.3g (bound %.3g)" % (q, worst, TOL))
    assert worst <= TOL, worst


def test_hostsim_rows_depend_on_their_own_recording_only(L, hostsim):
    """A recording alone, and the batch in another order, give the values the batch gives; slots that share columns hold the same values."""
    fe = importlib.import_module(PKG + ".frontend")
    q = 3
    out, desc, _, _, _ = run_hostsim(hostsim, fe, range(len(BATCH)), q)
    for i in (2, 5, 7):
        alone = run_hostsim(hostsim, fe, (i,), q)[0]
        lo = int(desc[i, 0])
        assert np.array_equal(alone, out[lo:lo + alone.shape[0]]), BATCH[i]
    order = (8, 0, 7, 3)
    mixed, mdesc, _, _, _ = run_hostsim(hostsim, fe, order, q)
    for r, i in enumerate(order):
        lo, mlo, n = int(desc[i, 0]), int(mdesc[r, 0]), fe.timeline_counts(BATCH[i], q)[1]
        assert np.array_equal(mixed[mlo:mlo + n], out[lo:lo + n]), BATCH[i]
    # the rows of a long recording are consecutive slots at q <= 10: slot u + 1's first 64 columns are slot u's last 64
    lo, n_slots = int(desc[8, 0]), fe.timeline_counts(BATCH[8], q)[1]
    assert n_slots > 10
    for r in range(lo, lo + n_slots - 1):
        assert np.array_equal(out[r][:, 32:], out[r + 1][:, :64])


def test_hostsim_refuses_what_the_library_refuses(L, hostsim):
    fe = importlib.import_module(PKG + ".frontend")
    desc, _, total, most = fe.timeline_descriptors([70000, 20000], 3)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rows = np.zeros((2, most), dtype=np.float32)
    out = np.zeros((total, 64, 96), dtype=np.float32)
    writes = np.zeros(out.shape, dtype=np.int32)
    computed = np.zeros((2, 384), dtype=np.int32)
    mr = np.zeros(2, dtype=np.int64)

    def run(d, n=most, slots=total):
        return hostsim.hostsim_logmel_timeline(p(rows), 2, n, most, p(d), slots, p(out), p(writes), p(computed), 384, p(mr))

    assert run(desc) == 0 and (writes == 1).all()
    writes[:] = 0
    assert run(desc, n=most - 1) == -14                      # recording 0 reads all of its row
    assert run(desc, slots=total + 1) == -1
    # -(10 (r + 1) + k): check k of logmel_timeline::check_rec fails for recording r
    for rec, field, value, code in ((0, 4, 0, -11), (0, 1, 385, -12), (0, 2, 100, -13), (0, 0, 1, -15), (0, 3, 8, -16), (1, 2, 97, -23),
                                    (1, 0, 9, -25), (1, 3, 47, -26)):
        bad = desc.copy()
        bad[rec, field] = value
        assert run(bad) == code, (rec, field, value)
    assert not writes.any()


def test_argument_errors_are_reported_before_any_launch(L):
    lib = L.lib()
    fe = importlib.import_module(PKG + ".frontend")
    for name in ("mla_timeline_counts", "mla_logmel_timeline", "mla_gather_bags"):
        assert name in L.declared_symbols()
    vp = ctypes.c_void_p
    fake = vp(0x1000)                                    # device pointers: never dereferenced, every call below fails validation first
    E_ARG, E_SHAPE, E_DTYPE = -1, -2, -5
    good, _, good_total, good_most = fe.timeline_descriptors([70000, 20000], 3)

    def timeline(pcm=fake, pcm_dtype=0, recordings=2, n_samples=good_most, row_stride=good_most, dev_desc=fake, desc=good, host=True,
                 total=good_total, tables=fake, out=fake, out_dtype=0):
        hd = np.ascontiguousarray(desc, dtype=np.int64)
        return lib.mla_logmel_timeline(pcm, pcm_dtype, recordings, n_samples, row_stride, dev_desc, hd.ctypes.data_as(vp) if host else None,
                                       total, tables, out, out_dtype, None)

    def expect(code, rc, needle=None):
        assert rc == code, (rc, lib.mla_last_error())
        if needle:
            assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    def with_field(rec, field, value):
        d = good.copy()
        d[rec, field] = value
        return d

    for null in ("pcm", "dev_desc", "tables", "out"):
        expect(E_ARG, timeline(**{null: None}), "null")
    expect(E_ARG, timeline(host=False), "null")
    expect(E_ARG, timeline(recordings=-1), "bad recordings")
    expect(E_ARG, timeline(row_stride=good_most - 1), "stride")
    expect(E_ARG, timeline(desc=with_field(0, 4, 0)), "recording 0: hop_slots 0")
    expect(E_ARG, timeline(desc=with_field(1, 4, -3)), "recording 1: hop_slots -3")
    expect(E_ARG, timeline(desc=with_field(0, 1, 383)), "are no track")
    expect(E_ARG, timeline(desc=with_field(0, 1, 384 + 32)), "are no track")          # not a whole hop of 96 columns
    expect(E_ARG, timeline(desc=with_field(1, 2, 95)), "are no track")
    expect(E_ARG, timeline(desc=with_field(1, 0, 0)), "recording 1: first_slot 0")
    expect(E_ARG, timeline(desc=with_field(1, 3, 0)), "first_item 0")
    expect(E_ARG, timeline(total=good_total - 1), "out has")
    expect(E_ARG, timeline(out=vp(0x1004)), "out must be 16-byte aligned")
    expect(E_ARG, timeline(dev_desc=vp(0x1004)), "desc 8-byte aligned")
    expect(E_ARG, timeline(tables=vp(0x1001)), "tables must be")
    expect(E_ARG, timeline(pcm=vp(0x1002)), "pcm misaligned")
    expect(E_SHAPE, timeline(n_samples=good_most - 1), "recording 0")                  # the long recording reads all of its row
    expect(E_SHAPE, timeline(desc=fe.timeline_descriptors([15600], 3)[0], recordings=1, total=10, n_samples=15599, row_stride=15600),
           "recording 0: 96 columns read 15600 samples, the rows hold 15599")
    for code in (1, 4, 7):
        expect(E_DTYPE, timeline(pcm_dtype=code), "pcm_dtype")
    for code in (2, 3, 6):
        expect(E_DTYPE, timeline(out_dtype=code), "out_dtype")
    assert timeline(recordings=0, total=0, pcm=None, dev_desc=None, host=False, tables=None, out=None) == 0
    assert timeline(recordings=0, total=0, pcm=None, dev_desc=None, host=False, tables=None, out=None, out_dtype=1, pcm_dtype=2) == 0
    expect(E_ARG, timeline(recordings=0, total=3), "no recordings but 3 slots")

    def gather(emb=fake, rows=40, ld=128, dev=fake, first=(0, 3, 30), host=True, windows=3, T=10, M=128, out=fake):
        fr = np.array(first, dtype=np.int64)
        return lib.mla_gather_bags(emb, rows, ld, dev, fr.ctypes.data_as(vp) if host else None, windows, T, M, out, None)

    for null in ("emb", "dev", "out"):
        expect(E_ARG, gather(**{null: None}), "null")
    expect(E_ARG, gather(host=False), "null")
    for bad in (dict(rows=-1), dict(windows=-1), dict(T=0), dict(M=0), dict(ld=127)):
        expect(E_ARG, gather(**bad), "bad gather_bags sizes")
    expect(E_ARG, gather(first=(0, 3, 31)), "window 2: rows 31 .. 40 leave emb (40 rows)")
    expect(E_ARG, gather(first=(-1, 3, 30)), "window 0")
    expect(E_ARG, gather(emb=vp(0x1002)), "misaligned")
    assert gather(windows=0, emb=None, dev=None, host=False, out=None) == 0


def test_python_errors_come_before_the_device_is_touched(L, tmp_path):
    import wave
    ds = importlib.import_module(PKG + ".dataset")
    torch = importlib.import_module("torch")
    ok = np.zeros(100000, dtype=np.float32)
    with pytest.raises(ValueError, match=r"recording 1: negative dimensions are not allowed \(239 samples at 16 kHz\)"):
        ds.recordings_to_slots([ok, np.zeros(239, dtype=np.float32)], 16000)
    with pytest.raises(ValueError, match=r"recording 0: negative dimensions"):
        ds.recordings_to_slots([np.zeros((717, 2), dtype=np.float32)], [48000])          # 239 samples at 16 kHz
    for q in (0, -2, 1.5):
        with pytest.raises(ValueError, match="hop_slots must be an integer >= 1"):
            ds.recordings_to_slots([ok], 16000, hop_slots=q)
    with pytest.raises(ValueError, match="2 recordings but 1 rates"):
        ds.recordings_to_slots([ok, ok], [44100])
    with pytest.raises(TypeError, match="all int16 or all floating"):
        ds.recordings_to_slots([ok, np.zeros(16000, dtype=np.int16)], 44100)
    # the clips launch's limit, stated in the docstring: refused from the lengths alone
    with pytest.raises(ValueError, match="more than one clips launch tiles"):
        ds._timeline_lengths([2 ** 31 + 100000], [16000], 3)
    with pytest.raises(ValueError, match="more than one clips launch tiles"):
        ds._timeline_lengths([2 ** 30] * 600, [16000] * 600, 3)
    n16, most = ds._timeline_lengths([176400, 8000, 700000], [44100, 8000, 16000], 3)
    assert n16.tolist() == [64000, 16000, 700000] and most == ds.timeline_counts(700000, 3)[2]
    for fn, args in ((ds.recordings_to_slots, ([], [])), (ds.wavfiles_to_slots, ([],)), (ds.audiofiles_to_slots, ([],))):
        slots, first_rows, index, starts = fn(*args, hop_slots=2, out_dtype=torch.bfloat16)
        assert tuple(slots.shape) == (0, 64, 96) and slots.dtype == torch.bfloat16
        assert first_rows.shape == index.shape == starts.shape == (0,) and starts.dtype == np.float64

    path = str(tmp_path / "short.wav")
    with wave.open(path, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(16000)
        wf.writeframes(bytes(2 * 239))
    for fn in (ds.wavfiles_to_slots, ds.audiofiles_to_slots):
        with pytest.raises(ValueError, match=r"recording 0: negative dimensions"):
            fn([path])


def test_timeline_entries_refuse_what_they_do_not_do():
    M = importlib.import_module(PKG + ".model")
    conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    rec = [np.zeros(100000, dtype=np.float32)]
    rn = M.Ensemble("repeat", conf, [2, 1], "cpu").eval()
    with pytest.raises(NotImplementedError, match=r"score_timeline scores .* use forward_recordings\(\)"):
        rn.score_timeline(rec, [16000])
    with pytest.raises(NotImplementedError, match="score_timeline_wavfiles"):
        rn.score_timeline_wavfiles(["nothing.wav"])
    with pytest.raises(NotImplementedError, match="score_timeline_audiofiles"):
        rn.score_timeline_audiofiles(["nothing.wav"])
    vg = M.Ensemble("repeat", dict(conf, cnn_type="vggish"), [2, 1], "cpu")
    assert vg.training
    for call in (lambda: vg.score_timeline(rec, [16000]), lambda: vg.score_timeline_wavfiles(["nothing.wav"]),
                 lambda: vg.score_timeline_audiofiles(["nothing.wav"])):
        with pytest.raises(RuntimeError, match="eval mode only"):
            call()
    vg.eval()
    with pytest.raises(ValueError, match="max_slots must be >= 1"):
        vg.score_timeline(rec, [16000], max_slots=0)
    six = M.Ensemble("repeat", dict(conf, cnn_type="vggish"), [2, 1], "cpu", slots=6).eval()
    with pytest.raises(ValueError, match="score_timeline builds the dataset's bags of 10 windows, the model takes slots = 6"):
        six.score_timeline(rec, [16000])
    # the one-bag entries keep refusing more than four examples
    ds = importlib.import_module(PKG + ".dataset")
    with pytest.raises(ValueError, match=r"could not broadcast input array from shape \(6,96,64\)"):
        ds.recordings_to_frames(rec, 16000)
