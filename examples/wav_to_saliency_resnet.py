#!/usr/bin/env python3
"""A WAV file -> the ResNet branch's top class and, per 224 x 224 mel-dB image of the 4 s clip, the time-frequency cell that moved
that class's score most: the cell of largest |gradient| of the images (clf.saliency_clips: the mel-dB front-end, the eval-mode
ResNet-50 trunk and the head forward, then the head's gradient behind autograd and the trunk walked back by hand down to
mla_rn_stem_dgrad; no weight gradient is launched).

    python examples/wav_to_saliency_resnet.py [--target K] [--bf16] [checkpoint.pt] [a.wav]

The file must be 16-bit PCM (any rate and channel count: it is mixed to mono, resampled to 22 050 Hz, cut at 4 s or zero-filled).
Without a WAV file it writes a synthetic one (three tone bursts) to a temporary directory. Without a checkpoint the weights are
seeded and the BatchNorm statistics are first moved to dB-scale images by a few train-mode passes over the clip and a clip of
noise, so the class only shows that the path runs. Text output, no plotting library."""

import importlib
import os
import sys
import tempfile
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "audio-classification-using-a-deep-cnn-combined-with-multi-level-attention_amd"
M = importlib.import_module(PKG + ".model")
W = importlib.import_module(PKG + ".weights")
DS = importlib.import_module(PKG + ".dataset")

RATE, SAMPLES, HOP = 22050, 88200, 98


def synthetic(directory):
    t = np.arange(4 * RATE) / float(RATE)
    x = sum(np.sin(2 * np.pi * f * t) * ((t > a) & (t < a + 0.8)) for f, a in ((440.0, 0.2), (1760.0, 1.5), (3520.0, 2.9)))
    x = x + 0.01 * np.random.default_rng(0).standard_normal(t.shape[0])       # a noise floor under the bursts
    path = os.path.join(directory, "bursts_22k_mono.wav")
    with wave.open(path, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(RATE)
        wf.writeframes((x * 12000).astype(np.int16).tobytes())
    return path


def main():
    args = sys.argv[1:]
    target = None
    if args and args[0] == "--target":
        target = int(args[1])
        args = args[2:]
    precision = "f32"
    if args and args[0] == "--bf16":
        precision = "bf16"
        args = args[1:]
    checkpoint = args.pop(0) if args and args[0].endswith(".pt") else None
    conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    clf = M.Ensemble("repeat", conf, [2, 1], torch.device("cuda"), precision=precision)
    sd = torch.load(checkpoint, map_location="cpu") if checkpoint else W.make_state_dict(21, W.ensemble_shapes((2, 1), True, cnn_type="resnet"))
    clf.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    clf.cuda()
    with tempfile.TemporaryDirectory() as tmp:
        path = args[0] if args else synthetic(tmp)
        pcm = DS.wavfiles_to_clips([path])
    if not checkpoint:                                   # seeded statistics describe unit-scale inputs, dB images are a hundred times larger
        calib = DS.clips_to_images(torch.cat([pcm, torch.rand(1, SAMPLES, device="cuda") - 0.5]))
        clf.train()
        with torch.no_grad():
            for _ in range(30):
                clf(calib)
    clf.eval()
    scores, images, grad = clf.saliency_clips(pcm, target=target)
    k = int(scores[0].argmax()) if target is None else target
    print("%s: class %d (score %.3f)%s" % (os.path.basename(path), k, float(scores[0, k]), "" if target is None else " [asked for]"))
    cells = grad[0, :, 0].abs().flatten(1)                               # (10, 224 * 224): band-major, frame-minor
    total = float(cells.sum())
    for e in range(images.shape[1]):
        at = int(cells[e].argmax())
        band, col = at // 224, at % 224
        print("  image %d: largest |grad| %.3e at mel band %3d of 224, column %3d (%.3f s into the image); share of the map %4.1f %%"
              % (e, float(cells[e, at]), band, col, col * HOP / float(RATE), 100.0 * float(cells[e].sum()) / total if total else 0.0))


if __name__ == "__main__":
    main()
