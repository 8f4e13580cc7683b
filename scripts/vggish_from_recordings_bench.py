#!/usr/bin/env python3
"""What the VGGish branch's batched path from recordings costs (dataset.recordings_to_frames, csrc/logmel.hip logmel_bags_kernel):
stereo int16 recordings at 44.1 kHz in host memory, as a set of four-second ones ("full") and a set with lengths drawn uniformly from
0.5 to 4 s ("ragged": what skipping absent 0.96 s examples gives), timed alternately round by round in one process on one device
(warm-up rounds first; median, minimum and maximum):

    batched    recordings_to_frames: two launches for the batch (host clock around work that ends in a device synchronise)
    loop       what a caller had to write before, per recording: waveform_to_examples with wavfile_to_examples' int16 scaling, then
               the create_spec + split re-framing (dataset._frames) (host clock, as above)
    bags       frontend.logmel_bags on the batch's clips into a preallocated output, by device events around the call: the kernel
               and the copy of its counts
    two        frontend.waveforms_to_examples + mla_dataset_frames on the same zero-filled clips into preallocated outputs, by
               device events around the two launches: the two kernels clips_to_frames runs, which compute all four examples of
               every row, and the gap between them
    forward    Ensemble.forward_recordings_native (bf16, seeded weights), host clock: `share` is batched / forward

The rows of batched and loop are compared bit for bit (batched_equals_loop). Prints one JSON line and, with --out FILE, writes it there.

    python scripts/vggish_from_recordings_bench.py [--sizes 64,512] [--rounds 20] [--warmup 3] [--out profiles/vggish_from_recordings.json]
"""

import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "audio-classification-using-a-deep-cnn-combined-with-multi-level-attention_amd"
DS = importlib.import_module(PKG + ".dataset")
FE = importlib.import_module(PKG + ".frontend")
LIB = importlib.import_module(PKG + "._lib")
VI = importlib.import_module(PKG + ".torchvggish.vggish_input")
M = importlib.import_module(PKG + ".model")
W = importlib.import_module(PKG + ".weights")

RATE, CHANNELS = 44100, 2


def recordings(kind, files):
    rng = np.random.default_rng(17 if kind == "full" else 18)
    frames = [4 * RATE] * files if kind == "full" else [int(n) for n in rng.uniform(0.5, 4.0, size=files) * RATE]
    return [rng.integers(-16000, 16001, size=(n, CHANNELS)).astype(np.int16) for n in frames]


def loop(recs):
    out = []
    for x in recs:
        ex = VI.waveform_to_examples(x, RATE, _pcm16=True).detach().reshape(-1, 96, 64)
        out.append(DS._frames(ex, 1, ex.shape[0], 10, 96, 32)[0])
    return torch.stack(out)[:, :, None]


def by_events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,512")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the GPU path; there is nothing to time without one"
    conf = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=1)
    ens = M.Ensemble("repeat", conf, [2, 1], torch.device("cuda"), precision="bf16")
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(6, W.ensemble_shapes((2, 1), False)).items()})
    ens.cuda().eval()
    stat = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    results = []
    for files in [int(s) for s in args.sizes.split(",")]:
        for kind in ("full", "ragged"):
            recs = recordings(kind, files)
            clips = DS.recordings_to_clips(recs, RATE, DS.SR_VGGISH, DS.SAMPLES_NUM_VGGISH)
            counts = DS._bag_counts([x.shape[0] for x in recs], [RATE] * files)
            same = bool(torch.equal(DS.recordings_to_frames(recs, RATE), loop(recs)))

            def forward():
                with torch.no_grad():
                    ens.forward_recordings_native(recs, RATE)

            # outputs allocated once: the event intervals below hold the launches (and logmel_bags' copy of its counts), no allocation
            bags_out = torch.empty((files, 10, 1, 64, 96), dtype=torch.float32, device=clips.device)
            ex_out = torch.empty((files * 4, 96, 64), dtype=torch.float32, device=clips.device)
            two_out = torch.empty((files, 10, 64, 96), dtype=torch.float32, device=clips.device)
            vp = ctypes.c_void_p

            def two():
                FE.waveforms_to_examples(clips, out=ex_out)
                LIB.check(LIB.lib().mla_dataset_frames(vp(ex_out.data_ptr()), files, 4, 10, 96, 32, vp(two_out.data_ptr()), LIB.stream_ptr()))

            host_ways = (("batched", lambda: DS.recordings_to_frames(recs, RATE)), ("loop", lambda: loop(recs)), ("forward", forward))
            event_ways = (("bags", lambda: FE.logmel_bags(clips, counts, 10, 32, out=bags_out)), ("two", two))
            ms = {n: [] for n, _ in host_ways}
            us = {n: [] for n, _ in event_ways}
            for r in range(args.warmup + args.rounds):
                for name, fn in host_ways:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if r >= args.warmup:
                        ms[name].append((time.perf_counter() - t0) * 1e3)
                for name, fn in event_ways:
                    e0, e1 = by_events(fn)
                    torch.cuda.synchronize()
                    if r >= args.warmup:
                        us[name].append(e0.elapsed_time(e1) * 1e3)
            results.append({"set": kind, "recordings": files, "examples": int(counts.sum()), "of": 4 * files, "batched_equals_loop": same,
                            "two_equals_bags_on_full_rows": bool(kind != "full" or torch.equal(two_out, bags_out[:, :, 0])),
                            "ms": {n: stat(v) for n, v in ms.items()}, "events_us": {n: stat(v) for n, v in us.items()},
                            "share_of_forward": round(statistics.median(ms["batched"]) / statistics.median(ms["forward"]), 3)})
    line = {"metric": "vggish_from_recordings", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "recording": "stereo int16 at 44.1 kHz, host memory", "rounds": args.rounds, "warmup": args.warmup, "results": results}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
