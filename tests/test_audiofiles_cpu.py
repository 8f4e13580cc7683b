"""WAV files of any PCM width or IEEE float -> clips, without a GPU: the RIFF reader and the host decoder (dataset.read_audiofile,
decode_audiofile) against scipy.io.wavfile, the refusals, the kernel's decode of file bytes simulated on the host workgroup by workgroup
(csrc/clips_hostsim.cpp, hostsim_clips_prepare_raw) on a batch of mixed encodings against the float64 chain of test_clips_cpu.py, the
C ABI's argument errors, and the pins of the 16-bit-only entries.

The bound is test_clips_cpu.py's TOL (2e-6 absolute) unchanged: every signal here stays inside +-0.5 of full scale in its encoding, and
the chain starts from the same decoded samples (scipy's, scaled in float64), so the coarse 8-bit quantisation is part of the input, not
of the error. Every file is written by this module: scipy.io.wavfile.write where it can, struct for 24-bit, extensible and broken ones."""

import ctypes
import importlib
import os
import struct

import numpy as np
import pytest
from scipy.io import wavfile

from conftest import PKG
from test_clips_cpu import CASES, PASSTHROUGH, SAMPLES_NUMS, SR_OUT, TOL, cut_and_fill, resampled_f64, run_hostsim
from test_clips_cpu import hostsim  # noqa: F401  (the fixture: one build of csrc/clips_hostsim.cpp for both modules' tests)

F32, I16, F64, I32, U8, I24 = 0, 2, 4, 5, 6, 7
BYTES = {U8: 1, I16: 2, I24: 3, I32: 4, F32: 4, F64: 8}
NAMES = {U8: "u8", I16: "i16", I24: "i24", I32: "i32", F32: "f32", F64: "f64"}
GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")            # KSDATAFORMAT_SUBTYPE_*: the tag (2 bytes) + these 14


def riff(path, tag, bits, channels, rate, payload, align=None, extensible=False, before_data=b"", declared=None, form=b"RIFF",
         wave=b"WAVE", data_first=False, with_data=True):
    """A RIFF/WAVE file assembled by hand; `payload` is the data chunk's bytes as they are."""
    align = channels * bits // 8 if align is None else align
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * align, align, bits)
    if extensible:
        fmt += struct.pack("<HHIH", 22, bits, 0, tag) + GUID_TAIL
        assert len(fmt) == 40
    fmt = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    data = b"data" + struct.pack("<I", len(payload) if declared is None else declared) + payload + b"\x00" * (len(payload) & 1)
    body = wave + (data + fmt if data_first else fmt + before_data + (data if with_data else b""))
    with open(path, "wb") as f:
        f.write(form + struct.pack("<I", len(body)) + body)
    return str(path)


def chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + b"\x00" * (len(body) & 1)


def i24_bytes(x):
    """int32 values in [-2**23, 2**23) -> packed little-endian 3-byte samples."""
    return np.ascontiguousarray(x.astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


def make_samples(code, n, channels, seed):
    """Seeded samples inside +-0.5 of full scale, (n, channels), in the dtype scipy reads the encoding as (24-bit: the int32 values
    before left-justification)."""
    rng = np.random.default_rng(seed)
    if code == U8:
        return rng.integers(64, 193, size=(n, channels)).astype(np.uint8)
    if code == I16:
        return rng.integers(-16000, 16001, size=(n, channels)).astype(np.int16)
    if code == I24:
        return rng.integers(-4000000, 4000001, size=(n, channels)).astype(np.int32)
    if code == I32:
        return rng.integers(-2 ** 30, 2 ** 30 + 1, size=(n, channels)).astype(np.int32)
    x = rng.uniform(-0.5, 0.5, size=(n, channels))                 # float64 samples are NOT float32 values: the rounding is exercised
    return x.astype(np.float32) if code == F32 else x


def write_file(path, code, rate, x):
    if code == I24:
        return riff(path, 1, 24, x.shape[1], rate, i24_bytes(x.reshape(-1)))
    wavfile.write(str(path), rate, x[:, 0] if x.shape[1] == 1 else x)
    return str(path)


def scipy_f64(path):
    """The independent decoder: scipy's samples scaled in float64 by the table of DESIGN.md 3.9, (rate, (n, channels))."""
    rate, x = wavfile.read(path)
    x = x.reshape(x.shape[0], -1)
    if x.dtype == np.uint8:
        y = (x.astype(np.float64) - 128.0) / 128.0
    elif x.dtype == np.int16:
        y = x.astype(np.float64) / 32768.0
    elif x.dtype == np.int32:                                       # 24-bit comes left-justified in int32
        y = x.astype(np.float64) / 2147483648.0
    else:
        assert x.dtype in (np.float32, np.float64), x.dtype
        y = x.astype(np.float32).astype(np.float64)
    return rate, y


def squeeze(y):
    return y[:, 0] if y.shape[1] == 1 else y


# the mixed batch: (encoding, (sr_in, channels, n_in, n_res)); CASES 0-5 with one encoding each, two recordings already at 22 050 Hz,
# and the 100-frame recording that is shorter than a filter wing. Row 3 is the multi-channel 32-bit PCM one.
MIXED = ((I24, CASES[0]), (F32, CASES[1]), (U8, CASES[2]), (I32, CASES[3]), (F64, CASES[4]), (I16, CASES[5]),
         (U8, PASSTHROUGH[0]), (I32, PASSTHROUGH[1]), (I16, CASES[6]))
MULTI_I32 = 3

_mixed = {}


def mixed_batch(directory):
    """Writes the mixed batch once per session; [(path, code, sr_in, channels, n_in, n_res)]."""
    if "files" not in _mixed:
        files = []
        for i, (code, (sr_in, ch, n, n_res)) in enumerate(MIXED):
            path = write_file(os.path.join(str(directory), "%d_%s.wav" % (i, NAMES[code])), code, sr_in, make_samples(code, n, ch, 2000 + i))
            files.append((path, code, sr_in, ch, n, n_res))
        _mixed["files"] = files
    return _mixed["files"]


def mixed_chain(directory):
    """float64 chain of every file of the batch before the cut (mean in double of scipy's decoded samples, rounded to float32 as the
    kernel's mono mix is, oracle/resample.py); computed once, shared with the GPU tests, never modified."""
    if "chain" not in _mixed:
        rows = []
        for path, _, sr_in, _, _, n_res in mixed_batch(directory):
            rate, y = scipy_f64(path)
            assert rate == sr_in
            r = resampled_f64(y, sr_in)
            assert len(r) == n_res
            r.setflags(write=False)
            rows.append(r)
        _mixed["chain"] = rows
    return _mixed["chain"]


def check_mixed_rows(got, directory, samples_num, what):
    worst = 0.0
    for i, ((path, code, sr_in, _, _, n_res), y) in enumerate(zip(mixed_batch(directory), mixed_chain(directory))):
        err = float(np.abs(got[i].astype(np.float64) - cut_and_fill(y, samples_num)).max())
        worst = max(worst, err)
        print("%s, samples_num %d, row %d (%s, %d Hz): |d| %.3g (bound %.3g)" % (what, samples_num, i, NAMES[code], sr_in, err, TOL))
        assert np.isfinite(got[i]).all() and err <= TOL, (what, path, samples_num, err)
        k = min(n_res, samples_num)
        assert not got[i, k:].any() and not np.signbit(got[i, k:]).any(), (what, path, "tail")
        if sr_in == SR_OUT:
            assert np.array_equal(got[i, :k], y[:k].astype(np.float32)), (what, path, "passthrough")
    return worst


@pytest.fixture(scope="module")
def ds():
    return importlib.import_module(PKG + ".dataset")


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def batch_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("audiofiles")


# ---- 1. the reader against scipy ----

@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("code", [U8, I16, I24, I32, F32, F64])
def test_reader_and_decoder_match_scipy(ds, tmp_path, code, channels):
    L = importlib.import_module(PKG + "._lib")
    assert (L.F32, L.I16, L.F64, L.I32, L.U8, L.I24) == (F32, I16, F64, I32, U8, I24)
    n, rate = 301, (8000, 44100, 96000)[channels - 1]
    path = write_file(tmp_path / "x.wav", code, rate, make_samples(code, n, channels, 10 * code + channels))
    data, desc = ds.read_audiofile(path)
    assert desc == (code, channels, rate, n)
    assert data.dtype == np.uint8 and data.shape == (n * channels * BYTES[code],)
    got, got_rate = ds.decode_audiofile(path)
    _, want = scipy_f64(path)
    assert got_rate == rate and got.dtype == np.float32 and got.shape == ((n,) if channels == 1 else (n, channels))
    assert np.array_equal(got, squeeze(want).astype(np.float32))
    assert np.abs(got).max() <= 0.5 + 1e-6 and np.abs(got).max() > 0.4


def test_extensible_headers(ds, tmp_path):
    x = make_samples(I24, 200, 2, 31)
    path = riff(tmp_path / "e24.wav", 1, 24, 2, 48000, i24_bytes(x.reshape(-1)), extensible=True)
    assert ds.read_audiofile(path)[1] == (I24, 2, 48000, 200)
    rate, want = scipy_f64(path)
    assert rate == 48000 and np.array_equal(ds.decode_audiofile(path)[0], want.astype(np.float32))
    assert np.array_equal(ds.decode_audiofile(path)[0], (x / 8388608.0).astype(np.float32))
    f = make_samples(F32, 150, 1, 32)
    path = riff(tmp_path / "ef32.wav", 3, 32, 1, 16000, f.tobytes(), extensible=True)
    assert ds.read_audiofile(path)[1] == (F32, 1, 16000, 150)
    assert np.array_equal(ds.decode_audiofile(path)[0], f[:, 0]) and np.array_equal(squeeze(scipy_f64(path)[1]).astype(np.float32), f[:, 0])


def test_chunk_walk_and_short_files(ds, tmp_path):
    x = make_samples(I16, 100, 2, 33)
    # an odd-sized LIST chunk (and its pad byte) and an unknown chunk before the data
    path = riff(tmp_path / "list.wav", 1, 16, 2, 32000, x.tobytes(), before_data=chunk(b"LIST", b"INFOabc") + chunk(b"bext", b"\x01" * 10))
    assert ds.read_audiofile(path)[1] == (I16, 2, 32000, 100)
    assert np.array_equal(ds.decode_audiofile(path)[0], x.astype(np.float32) / 32768)
    assert np.array_equal(squeeze(scipy_f64(path)[1]), x / 32768.0)
    # the declared data size exceeds the bytes present: the frames that are there
    path = riff(tmp_path / "trunc.wav", 1, 16, 2, 32000, x.tobytes()[:4 * 60], declared=400000)
    data, desc = ds.read_audiofile(path)
    assert desc == (I16, 2, 32000, 60) and data.tobytes() == x.tobytes()[:240]
    assert np.array_equal(ds.decode_audiofile(path)[0], x[:60].astype(np.float32) / 32768)
    # a trailing partial frame, declared and present: only the incomplete frame is lost
    x24 = make_samples(I24, 50, 2, 34)
    path = riff(tmp_path / "partial.wav", 1, 24, 2, 44100, i24_bytes(x24.reshape(-1))[:6 * 40 + 4])
    data, desc = ds.read_audiofile(path)
    assert desc == (I24, 2, 44100, 40) and data.shape == (240,)
    assert np.array_equal(ds.decode_audiofile(path)[0], (x24[:40] / 8388608.0).astype(np.float32))
    # truncated in the middle of a frame with a larger declared size
    path = riff(tmp_path / "both.wav", 3, 64, 1, 8000, make_samples(F64, 20, 1, 35).tobytes()[:8 * 7 + 5], declared=160)
    assert ds.read_audiofile(path)[1] == (F64, 1, 8000, 7)
    # a data chunk with nothing in it
    path = riff(tmp_path / "none.wav", 1, 8, 1, 8000, b"")
    data, desc = ds.read_audiofile(path)
    assert desc == (U8, 1, 8000, 0) and data.shape == (0,) and ds.decode_audiofile(path)[0].shape == (0,)


# ---- 2. refusals ----

def test_refusals_name_the_path(ds, tmp_path):
    pay = b"\x00" * 64
    cases = {
        "adpcm": dict(tag=2, bits=4, align=256), "ima": dict(tag=0x11, bits=4, align=256), "alaw": dict(tag=6, bits=8),
        "mulaw": dict(tag=7, bits=8), "mp3": dict(tag=0x55, bits=0, align=1), "rifx": dict(tag=1, bits=16, form=b"RIFX"),
        "rf64": dict(tag=1, bits=16, form=b"RF64"), "pcm12": dict(tag=1, bits=12, align=2), "f16": dict(tag=3, bits=16),
        "nodata": dict(tag=1, bits=16, with_data=False), "datafirst": dict(tag=1, bits=16, data_first=True),
        "align": dict(tag=1, bits=16, align=4), "ext_mulaw": dict(tag=7, bits=8, extensible=True), "form": dict(tag=1, bits=16, wave=b"AVI "),
        "gsm": dict(tag=0x31, bits=0, align=65),
    }
    needles = {"adpcm": "ADPCM", "ima": "ADPCM", "alaw": "A-law", "mulaw": "mu-law", "mp3": "MP3", "pcm12": "12-bit", "f16": "16-bit",
               "nodata": "no data", "datafirst": "before", "align": "block align", "rifx": "RIFF", "rf64": "RIFF", "gsm": "0x0031"}
    for name, kw in cases.items():
        kw = dict(kw)
        path = riff(tmp_path / (name + ".wav"), kw.pop("tag"), kw.pop("bits"), 1, 8000, pay, **kw)
        for fn in (ds.read_audiofile, ds.decode_audiofile, lambda p: ds.audiofiles_to_clips([p])):
            with pytest.raises(ValueError) as e:
                fn(path)
            assert path in str(e.value) and needles.get(name, "") in str(e.value), (name, str(e.value))
    for name, ch, rate in (("zero_channels", 0, 8000), ("zero_rate", 1, 0)):
        path = riff(tmp_path / (name + ".wav"), 1, 16, ch, rate, pay, align=2)
        with pytest.raises(ValueError) as e:
            ds.read_audiofile(path)
        assert path in str(e.value), name
    for name, content in (("empty", b""), ("short", b"RIFF\x04\x00\x00\x00WAV"), ("tiny_fmt", b"RIFF\x14\x00\x00\x00WAVEfmt \x08\x00\x00\x00" + b"\x01" * 8)):
        path = str(tmp_path / (name + ".wav"))
        with open(path, "wb") as f:
            f.write(content)
        with pytest.raises(ValueError) as e:
            ds.read_audiofile(path)
        assert path in str(e.value), name
    with pytest.raises(OSError):
        ds.read_audiofile(str(tmp_path / "missing.wav"))


def test_python_errors_come_before_the_device_is_touched(ds, tmp_path):
    import torch
    ok = write_file(tmp_path / "ok.wav", I24, 44100, make_samples(I24, 500, 1, 41))
    two = write_file(tmp_path / "two.wav", F32, 48000, make_samples(F32, 2, 1, 42))
    with pytest.raises(ValueError, match=r"recording 1: Input signal length=2 is too small to resample from 48000->22050"):
        ds.audiofiles_to_clips([ok, two])
    with pytest.raises(ValueError, match="Invalid sample rate"):
        ds.audiofiles_to_clips([ok], sr=0)
    empty = ds.audiofiles_to_clips([])
    assert tuple(empty.shape) == (0, 88200) and empty.dtype == torch.float32
    assert tuple(ds.audiofiles_to_clips([], samples_num=2000).shape) == (0, 2000)


# ---- 3. the kernel on file bytes, simulated on the host ----

def _tables(fe, rates):
    rates = np.array(rates, dtype=np.float64)
    scales, tab = fe.clips_table_index(rates, float(SR_OUT))
    tables = fe.clips_tables_host(scales)
    return rates, tab, tables, (len(tables) // (2 * len(scales)) if scales else 32769)


def run_raw(hostsim, fe, ds, files, samples_num, guard):
    """Pack the files' data chunks (each on a multiple of 8 bytes, `guard` bytes of 0xFF before, between and after them: all-ones
    bytes are NaN as float32 and as float64, and -1 or 255 as PCM) and run the simulated launch of mla_clips_prepare_raw."""
    read = [ds.read_audiofile(f[0]) for f in files]
    sizes = [d.shape[0] for d, _ in read]
    offsets, pos = [], guard
    for s in sizes:
        offsets.append(pos)
        pos += (s + 7) // 8 * 8 + guard
    packed = np.full(pos if guard else offsets[-1] + sizes[-1], 0xFF, dtype=np.uint8)
    for (d, _), o, s in zip(read, offsets, sizes):
        packed[o:o + s] = d
    code, ch, rate, frames = (np.array(v) for v in zip(*(desc for _, desc in read)))
    rates, tab, tables, nwin = _tables(fe, rate)
    out = np.full((len(files), samples_num), np.nan, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    offsets, frames, ch, code = np.array(offsets, np.int64), frames.astype(np.int64), ch.astype(np.int32), code.astype(np.int32)
    cap = hostsim.hostsim_clips_prepare_raw(p(packed), len(files), p(offsets), p(frames), p(ch), p(code), p(rates), p(tab), float(SR_OUT),
                                            samples_num, p(tables), nwin, 512, p(out))
    assert cap >= 0, cap
    return out, cap


@pytest.mark.parametrize("samples_num", SAMPLES_NUMS)
def test_raw_kernel_math_on_host(hostsim, fe, ds, batch_dir, samples_num):
    files = mixed_batch(batch_dir)
    got, cap = run_raw(hostsim, fe, ds, files, samples_num, guard=0)
    assert cap == 3351                                                   # the 192 kHz recording's, as in test_clips_cpu.py
    check_mixed_rows(got, batch_dir, samples_num, "host simulation")    # (a) the bound, (c) the tails, passthrough
    # (d) 0xFF guard bytes around every recording never reach an output
    guarded, _ = run_raw(hostsim, fe, ds, files, samples_num, guard=64)
    assert np.isfinite(guarded).all() and np.array_equal(guarded.view(np.uint32), got.view(np.uint32))
    # (b) int16 and float32 recordings: the rows of the element-offset entry on the same samples
    for code, dtype in ((I16, np.int16), (F32, np.float32)):
        rows = [i for i, f in enumerate(files) if f[1] == code]
        recs = [squeeze(wavfile.read(files[i][0])[1].reshape(files[i][4], -1)) for i in rows]
        assert rows and all(r.dtype == dtype for r in recs)
        want, _ = run_hostsim(hostsim, fe, recs, [files[i][2] for i in rows], samples_num)
        for k, i in enumerate(rows):
            assert np.array_equal(got[i].view(np.uint32), want[k].view(np.uint32)), files[i][0]
    # every encoding but multi-channel 32-bit PCM: the rows of the element-offset entry on the float32 decode
    rows = [i for i in range(len(files)) if i != MULTI_I32]
    want, _ = run_hostsim(hostsim, fe, [ds.decode_audiofile(files[i][0])[0] for i in rows], [files[i][2] for i in rows], samples_num)
    for k, i in enumerate(rows):
        assert np.array_equal(got[i].view(np.uint32), want[k].view(np.uint32)), files[i][0]
    # a row depends on its own file only
    perm = [4, 8, 0, 6, 2, 7, 5, 3, 1]
    moved, _ = run_raw(hostsim, fe, ds, [files[i] for i in perm], samples_num, guard=8)
    for row, i in enumerate(perm):
        assert np.array_equal(moved[row].view(np.uint32), got[i].view(np.uint32)), (row, i)


def test_the_mixed_batch_is_what_it_says():
    assert [c for c, _ in MIXED[:6]].count(I24) == 1 and {c for c, _ in MIXED[:6]} == {U8, I16, I24, I32, F32, F64}
    assert MIXED[MULTI_I32][0] == I32 and MIXED[MULTI_I32][1][1] == 3
    assert [m[1][0] for m in MIXED[6:8]] == [SR_OUT, SR_OUT] and MIXED[8][1][2] == 100 < 32769 // 256
    assert all(m[1][1] == 1 for m in MIXED if m[0] == I32 and m is not MIXED[MULTI_I32])


# ---- 4. argument errors of the C entry ----

def test_raw_argument_errors_are_reported_before_any_launch(L):
    lib = L.lib()
    assert "mla_clips_prepare_raw" in L.declared_symbols()
    vp = ctypes.c_void_p
    fake = vp(0x1000)                                    # device pointers: never dereferenced, every call below fails validation first
    E_ARG, E_SHAPE, E_SHORT = -1, -2, -3

    # clip 0: 1000 mono frames of 24-bit at byte 0; clip 1: 2000 stereo frames of int16 at byte 3000
    def prepare(packed=fake, packed_bytes=11000, clips=2, dev=fake, frames=(1000, 2000), channels=(1, 2), rates=(44100.0, 22050.0),
                offsets=(0, 3000), tab=(0, 0), formats=(I24, I16), host=True, sr_out=22050.0, samples_num=2048, tables=fake, n_tables=1,
                nwin=32769, num_table=512, out=fake):
        arrs = [np.array(offsets, dtype=np.int64), np.array(frames, dtype=np.int64), np.array(channels, dtype=np.int32),
                np.array(rates, dtype=np.float64), np.array(tab, dtype=np.int32), np.array(formats, dtype=np.int32)]
        hp = [a.ctypes.data_as(vp) if host else None for a in arrs]
        return lib.mla_clips_prepare_raw(packed, packed_bytes, clips, dev, dev, dev, dev, dev, dev, *hp, sr_out, samples_num, tables,
                                         n_tables, nwin, num_table, out, None)

    def expect(code, rc, needle=None):
        assert rc == code, (rc, lib.mla_last_error())
        if needle:
            assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    for null in ("packed", "dev", "tables", "out"):
        expect(E_ARG, prepare(**{null: None}), "null")
    expect(E_ARG, prepare(host=False), "null")
    expect(E_ARG, prepare(clips=-1), "negative")
    expect(E_ARG, prepare(samples_num=-1), "negative")
    expect(E_ARG, prepare(packed_bytes=-1), "negative")
    expect(E_ARG, prepare(n_tables=-1), "negative")
    for bad in (1, 3, 8, -1, 100):                       # MLA_BF16, MLA_BF16X3 and numbers that are no code at all
        expect(E_ARG, prepare(formats=(I24, bad)), "clip 1: format code %d" % bad)
    expect(E_ARG, prepare(formats=(9, I16)), "clip 0")
    # an offset that is no multiple of the sample size, for each of the 2/4/8-byte formats; any offset suits 1- and 3-byte samples
    for code, size in ((I16, 2), (I32, 4), (F32, 4), (F64, 8)):
        for off in (3000 + 1, 3000 + size // 2, 3000 + size - 1):
            expect(E_ARG, prepare(formats=(I24, code), frames=(1000, 100), offsets=(0, off)), "misaligned")
    expect(E_SHORT, prepare(formats=(U8, I16), offsets=(1, 3000), frames=(1, 2000)), "too short")          # accepted as far as the offset goes
    expect(E_SHORT, prepare(formats=(I24, I16), offsets=(1, 3000), frames=(1, 2000)), "too short")
    expect(E_ARG, prepare(packed=vp(0x1004)), "aligned")
    # the last clip ends exactly at the buffer's end; one byte less and it leaves it
    expect(E_SHORT, prepare(frames=(1, 2000)), "too short")
    expect(E_ARG, prepare(packed_bytes=10999), "clip 1: bytes [3000, 11000) leave")
    expect(E_ARG, prepare(packed_bytes=2999, clips=1), "clip 0: bytes [0, 3000) leave")
    expect(E_ARG, prepare(offsets=(8002, 3000)), "clip 0: bytes [8002, 11002) leave")
    expect(E_ARG, prepare(offsets=(-3, 3000)), "leave")
    expect(E_ARG, prepare(formats=(I24, F64), channels=(1, 1), frames=(1000, 1001), offsets=(0, 3000)), "leave")
    expect(E_ARG, prepare(frames=(-1, 2000)), "clip 0")
    expect(E_ARG, prepare(channels=(1, 0)), "clip 1")
    expect(E_ARG, prepare(rates=(0.0, 22050.0)), "clip 0")
    expect(E_ARG, prepare(sr_out=0.0), "sr_out")
    expect(E_ARG, prepare(tab=(1, 0)), "table")
    expect(E_SHAPE, prepare(rates=(16.0 * 22050 + 1, 22050.0)), "16 x")
    expect(E_SHAPE, prepare(rates=(22050.0 * 513, 22050.0)), "resolution")
    assert prepare(clips=0, packed=None, dev=None, host=False, tables=None, out=None) == 0
    assert prepare(clips=0, packed=None, dev=None, host=False, tables=None, out=None, packed_bytes=0, n_tables=0) == 0


# ---- 5. and 6. the model's entry and the pins of the 16-bit-only entries ----

def test_forward_audiofiles_needs_the_resnet_branch():
    M = importlib.import_module(PKG + ".model")
    conf = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    vg = M.Ensemble("repeat", conf, [2, 1], "cpu")
    with pytest.raises(NotImplementedError, match="forward_audiofiles"):
        vg.forward_audiofiles(["nothing.wav"])


def test_the_16_bit_entries_still_refuse_other_widths(ds, tmp_path):
    eight = write_file(tmp_path / "eight.wav", U8, 22050, make_samples(U8, 3000, 1, 51))
    with pytest.raises(AssertionError, match="Bad sample type: 1"):
        ds.wavfiles_to_clips([eight])
    with pytest.raises(AssertionError, match="Bad sample type: 1"):
        ds.read_wav16(eight)
    with pytest.raises(TypeError, match="all int16 or all floating"):
        ds.recordings_to_clips([np.zeros(5000, dtype=np.float32), np.zeros(5000, dtype=np.int16)], 44100)
    with pytest.raises(TypeError, match="int16 or floating samples expected"):
        ds.recordings_to_clips([np.zeros(5000, dtype=np.int32)], 44100)
