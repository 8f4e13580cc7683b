#!/usr/bin/env python3
"""What decoding WAV files on the device costs or buys (dataset.audiofiles_to_clips, csrc/clips.hip clips_kernel on file bytes): one batch of
four-second stereo files at 44.1 kHz, written once to a temporary directory as 16-bit PCM, 24-bit PCM and float32 copies of the same
audio, and six ways from the first byte read to the (files, 88 200) clips tensor, timed alternately round by round in one process
on one device (host clock around work that ends in a device synchronise; warm-up rounds first; median, minimum and maximum):

    i16_raw    audiofiles_to_clips on the 16-bit files          i16_wave    wavfiles_to_clips on them (stdlib wave + recordings_to_clips)
    i24_raw    audiofiles_to_clips on the 24-bit files          i24_host    decode_audiofile per file + recordings_to_clips
    f32_raw    audiofiles_to_clips on the float32 files         f32_host    decode_audiofile per file + recordings_to_clips

The *_host ways are what a caller had to write before for files `wave` refuses. The kernel of every way alone comes from the device
events ops._timed records around its launch in the same rounds. The rows of each pair are compared bit for bit. Prints one JSON line
and, with --out FILE, writes it there.

    python scripts/audiofiles_bench.py [--files 64] [--rounds 25] [--warmup 3] [--out profiles/audiofiles_to_clips.json]
"""

import argparse
import importlib
import json
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "audio-classification-using-a-deep-cnn-combined-with-multi-level-attention_amd"
DS = importlib.import_module(PKG + ".dataset")
OPS = importlib.import_module(PKG + ".ops")

RATE, CHANNELS, FRAMES = 44100, 2, 4 * 44100


def write_wav(path, tag, bits, payload):
    align = CHANNELS * bits // 8
    fmt = struct.pack("<HHIIHH", tag, CHANNELS, RATE, RATE * align, align, bits)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(payload)) + b"WAVEfmt " + struct.pack("<I", len(fmt)) + fmt
                + b"data" + struct.pack("<I", len(payload)) + payload)


def write_files(directory, files):
    """The same seeded audio (amplitude 0.5) three times: 16-bit, 24-bit (the 16-bit samples left-justified, so that all three decode
    to the same float32 values) and float32."""
    paths = {"i16": [], "i24": [], "f32": []}
    for i in range(files):
        x = np.random.default_rng(i).integers(-16000, 16001, size=(FRAMES, CHANNELS)).astype("<i2")
        for kind, tag, bits, payload in (("i16", 1, 16, x.tobytes()),
                                         ("i24", 1, 24, (x.astype("<i4") << 8).view(np.uint8).reshape(-1, 4)[:, :3].tobytes()),
                                         ("f32", 3, 32, (x.astype("<f4") / np.float32(32768.0)).tobytes())):
            paths[kind].append(os.path.join(directory, "%s_%03d.wav" % (kind, i)))
            write_wav(paths[kind][-1], tag, bits, payload)
    return paths


def host_decoded(paths):
    decoded = [DS.decode_audiofile(p) for p in paths]
    return DS.recordings_to_clips([d[0] for d in decoded], [d[1] for d in decoded])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the GPU path; there is nothing to time without one"
    with tempfile.TemporaryDirectory() as directory:
        paths = write_files(directory, args.files)
        ways = (("i16_raw", lambda: DS.audiofiles_to_clips(paths["i16"])), ("i16_wave", lambda: DS.wavfiles_to_clips(paths["i16"])),
                ("i24_raw", lambda: DS.audiofiles_to_clips(paths["i24"])), ("i24_host", lambda: host_decoded(paths["i24"])),
                ("f32_raw", lambda: DS.audiofiles_to_clips(paths["f32"])), ("f32_host", lambda: host_decoded(paths["f32"])))
        rows = {name: fn() for name, fn in ways}
        torch.cuda.synchronize()
        same = {a + "_equals_" + b: bool(torch.equal(rows[a], rows[b])) for a, b in (("i16_raw", "i16_wave"), ("i24_raw", "i24_host"),
                                                                                    ("f32_raw", "f32_host"), ("i24_raw", "i16_raw"),
                                                                                    ("f32_raw", "i16_raw"))}
        del rows
        OPS.reserve_events(4)
        total, kernel = {n: [] for n, _ in ways}, {n: [] for n, _ in ways}
        for r in range(args.warmup + args.rounds):
            for name, fn in ways:
                OPS.reserve_events(2)
                OPS.profile = []
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                (_, e0, e1), = OPS.profile
                OPS.profile = None
                if r >= args.warmup:
                    total[name].append((t1 - t0) * 1e3)
                    kernel[name].append(e0.elapsed_time(e1) * 1e3)
    stat = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    line = {"metric": "audiofiles_to_clips", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "files": args.files, "recording": "4 s stereo at 44.1 kHz", "rounds": args.rounds, "warmup": args.warmup, **same,
            "bytes_uploaded_MB": {k: round(args.files * FRAMES * CHANNELS * b / 1e6, 1) for k, b in (("i16", 2), ("i24", 3), ("f32", 4))},
            "first_byte_to_clips_ms": {n: stat(v) for n, v in total.items()}, "kernel_us": {n: stat(v) for n, v in kernel.items()}}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
