#!/usr/bin/env python3
"""What scoring a long recording over time costs (Ensemble.score_timeline, csrc/logmel.hip logmel_timeline_kernel): one mono int16
recording at 16 kHz in host memory per length (60 s and 600 s by default), hop_slots = 3 (one window every 0.96 s), bf16, seeded
weights. Timed alternately round by round in one process on one device (warm-up rounds first; median, minimum and maximum):

    timeline   Ensemble.score_timeline: two front-end launches over the distinct slots, the CNN once per slot (3 W + 7 of them), one
               gather, the head (host clock around work that ends in a device synchronise)
    crops      what a caller had before: crop every window's 61 680 samples on the host and call forward_recordings_native on batches
               of --batch crops; the CNN runs on 10 W slots (host clock, as above)
    front      the two launches of dataset.recordings_to_slots alone, by the device events ops.profile records around each, with
               the bytes they move: the recording up, the 16 kHz row written and read, the slots written

At 16 kHz a host crop holds the very samples of its window, so the two routes' scores are compared bit for bit (timeline_equals_crops).
Prints one JSON line and, with --out FILE, writes it there.

    python scripts/timeline_bench.py [--seconds 60,600] [--batch 128] [--rounds 10] [--warmup 2] [--out profiles/timeline.json]
"""

import argparse
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
OPS = importlib.import_module(PKG + ".ops")
M = importlib.import_module(PKG + ".model")
W = importlib.import_module(PKG + ".weights")

RATE, Q, WINDOW, HOP = 16000, 3, 61680, 5120


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", default="60,600")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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
    for seconds in [int(s) for s in args.seconds.split(",")]:
        rec = np.random.default_rng(40 + seconds).integers(-16000, 16001, size=seconds * RATE).astype(np.int16)
        windows, slots, read = DS.timeline_counts(rec.shape[0], Q)

        def timeline():
            with torch.no_grad():
                return ens.score_timeline([rec], RATE, hop_slots=Q)[0]

        def crops():
            with torch.no_grad():
                out = []
                for w0 in range(0, windows, args.batch):
                    pieces = [rec[HOP * Q * w:HOP * Q * w + WINDOW] for w in range(w0, min(w0 + args.batch, windows))]
                    out.append(ens.forward_recordings_native(pieces, RATE))
                return torch.cat(out)

        same = bool(torch.equal(timeline(), crops()))
        ways = (("timeline", timeline), ("crops", crops))
        ms = {n: [] for n, _ in ways}
        front = {"clips_prepare": [], "logmel_timeline": []}
        for r in range(args.warmup + args.rounds):
            for name, fn in ways:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= args.warmup:
                    ms[name].append((time.perf_counter() - t0) * 1e3)
            OPS.reserve_events(4)
            OPS.profile = []
            try:
                DS.recordings_to_slots([rec], RATE, hop_slots=Q, out_dtype=torch.bfloat16)
                torch.cuda.synchronize()
                spans = [(n, e0.elapsed_time(e1) * 1e3) for n, e0, e1 in OPS.profile]
            finally:
                OPS.profile = None
            assert [n for n, _ in spans] == ["clips_prepare", "logmel_timeline"]
            if r >= args.warmup:
                for n, us in spans:
                    front[n].append(us)
        results.append({"seconds": seconds, "windows": windows, "cnn_slots": {"timeline": slots, "crops": 10 * windows},
                        "timeline_equals_crops": same, "ms": {n: stat(v) for n, v in ms.items()},
                        "speedup": round(statistics.median(ms["crops"]) / statistics.median(ms["timeline"]), 3),
                        "front_events_us": {n: stat(v) for n, v in front.items()},
                        "front_bytes": {"clips_prepare": 2 * rec.shape[0] + 4 * read, "logmel_timeline": 4 * read + 2 * slots * 64 * 96}})
    line = {"metric": "timeline", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "recording": "mono int16 at 16 kHz, host memory", "hop_slots": Q, "precision": "bf16", "crops_batch": args.batch,
            "rounds": args.rounds, "warmup": args.warmup, "results": results}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
