#!/usr/bin/env python3
"""What scoring a long recording over time costs on the ResNet branch (Ensemble.score_image_timeline, csrc/melspec.hip
melspec_track_*): one mono int16 recording at 22 050 Hz in host memory per length (60 s and 600 s by default), hop_images = 3 (one
window every second), bf16 and f32, seeded weights. Timed alternately round by round in one process on one device (warm-up rounds
first; median, minimum and maximum):

    timeline   Ensemble.score_image_timeline: the clips launch, the track's spectrogram and maximum once, then per chunk of
               max_images distinct images the images launch and the trunk (3 W + 7 images), one gather, the head (host clock around
               work that ends in a device synchronise)
    crops      what a caller had before: crop every window's 88 200 samples on the host and call forward_recordings on batches of
               --batch crops; front-end and trunk run on 10 W images (host clock, as above)
    front      the launches of dataset.recordings_to_track_images alone, by the device events ops.profile records around each, with
               the bytes they must move: the recording up and the row written; the track read and D written; D read and the images written

The two routes do NOT compute the same thing (the crop route reflects at every crop's ends and floors against
every crop's own maximum), so their scores are compared by their largest difference, not bit for bit. Prints one JSON line and,
with --out FILE, writes it there.

    python scripts/image_timeline_bench.py [--seconds 60,600] [--batch 25] [--rounds 3] [--warmup 1] [--out profiles/image_timeline.json]
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

RATE, Q, WINDOW, STEP = 22050, 3, 88200, 7350
FRONT = ("clips_prepare", "melspec_track_db", "melspec_track_images")


def model(precision):
    conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    ens = M.Ensemble("repeat", conf, [2, 1], torch.device("cuda"), precision=precision)
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(11, W.ensemble_shapes((2, 1), True, cnn_type="resnet")).items()})
    ens.cuda()
    # the seeded running statistics of the head describe unit-scale inputs; thirty train-mode passes over two other clips move them to
    # dB images (tests/test_melspec_gpu.py test_forward_clips), so that the scores the two routes are compared by are finite
    rng = np.random.default_rng(7)
    calib = DS.clips_to_images(DS.recordings_to_clips([rng.integers(-16000, 16001, size=WINDOW).astype(np.int16) for _ in range(2)], RATE))
    ens.train()
    with torch.no_grad():
        for _ in range(30):
            ens(calib)
    return ens.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", default="60,600")
    ap.add_argument("--precisions", default="bf16,f32")
    ap.add_argument("--batch", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the GPU path; there is nothing to time without one"
    stat = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}      # noqa: E731
    results = []
    for precision in args.precisions.split(","):
        ens = model(precision)
        for seconds in [int(s) for s in args.seconds.split(",")]:
            rec = np.random.default_rng(40 + seconds).integers(-16000, 16001, size=seconds * RATE).astype(np.int16)
            windows, images, samples, columns = DS.image_timeline_counts(rec.shape[0], Q)

            def timeline():
                with torch.no_grad():
                    return ens.score_image_timeline([rec], RATE, hop_images=Q)[0]

            def crops():
                with torch.no_grad():
                    out = []
                    for w0 in range(0, windows, args.batch):
                        pieces = [rec[STEP * Q * w:STEP * Q * w + WINDOW] for w in range(w0, min(w0 + args.batch, windows))]
                        out.append(ens.forward_recordings(pieces, RATE))
                    return torch.cat(out)

            a, b = timeline(), crops()
            finite = bool(torch.isfinite(a).all() and torch.isfinite(b).all())
            apart = float((a - b).abs().max()) if finite else None
            ways = (("timeline", timeline), ("crops", crops))
            ms = {n: [] for n, _ in ways}
            front = {n: [] for n in FRONT}
            for r in range(args.warmup + args.rounds):
                for name, fn in ways:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if r >= args.warmup:
                        ms[name].append((time.perf_counter() - t0) * 1e3)
                OPS.reserve_events(6)
                OPS.profile = []
                try:
                    DS.recordings_to_track_images([rec], RATE, hop_images=Q)
                    torch.cuda.synchronize()
                    spans = [(n, e0.elapsed_time(e1) * 1e3) for n, e0, e1 in OPS.profile]
                finally:
                    OPS.profile = None
                assert tuple(n for n, _ in spans) == FRONT
                if r >= args.warmup:
                    for n, us in spans:
                        front[n].append(us)
            results.append({"precision": precision, "seconds": seconds, "windows": windows, "cnn_images": {"timeline": images, "crops": 10 * windows},
                            "scores_finite": finite, "timeline_minus_crops_max_abs": apart, "ms": {n: stat(v) for n, v in ms.items()},
                            "speedup": round(statistics.median(ms["crops"]) / statistics.median(ms["timeline"]), 3),
                            "front_events_us": {n: stat(v) for n, v in front.items()},
                            "front_bytes": {"clips_prepare": 2 * rec.shape[0] + 4 * samples, "melspec_track_db": 4 * samples + 896 * columns,
                                            "melspec_track_images": 896 * columns + 4 * 224 * 224 * images}})
    line = {"metric": "image_timeline", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "recording": "mono int16 at 22 050 Hz, host memory", "hop_images": Q, "max_images": 256, "crops_batch": args.batch,
            "rounds": args.rounds, "warmup": args.warmup, "results": results}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
