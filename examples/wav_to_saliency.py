#!/usr/bin/env python3
"""A WAV file -> the top class and, per 0.96 s example, the time-frequency cell that moved that class's score most: the cell of
largest |gradient x input| of the log-mel examples (clf.saliency_waveforms: the log-mel front-end, the CNN and the head forward,
then the head's, the Linear layers' and the conv stack's data gradients down to mla_conv1_dgrad; no weight gradient is launched).

    python examples/wav_to_saliency.py [--target K] [checkpoint.pt] [a.wav]

The file must be 16-bit PCM at 16 kHz (channels are averaged); its first 9.6 s are one bag of ten examples, a shorter file is
zero-filled. Without a WAV file it writes a synthetic one (three tone bursts) to a temporary directory. Without a checkpoint the
weights are seeded, so the class only shows that the path runs. Text output, no plotting library."""

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

RATE, EXAMPLES = 16000, 10
SAMPLES = 15600 + (EXAMPLES - 1) * 15360            # what ten 0.96 s examples read (vggish_input.py:62-71)


def synthetic(directory):
    t = np.arange(10 * RATE) / float(RATE)
    x = sum(np.sin(2 * np.pi * f * t) * ((t > a) & (t < a + 1.5)) for f, a in ((440.0, 0.5), (1760.0, 3.5), (3520.0, 7.0)))
    path = os.path.join(directory, "bursts_16k_mono.wav")
    with wave.open(path, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(RATE)
        wf.writeframes((x * 12000).astype(np.int16).tobytes())
    return path


def read_16k(path):
    with wave.open(path, "rb") as wf:
        if wf.getsampwidth() != 2 or wf.getframerate() != RATE:
            raise SystemExit("%s: 16-bit PCM at 16 kHz wanted, got %d-bit at %d Hz" % (path, 8 * wf.getsampwidth(), wf.getframerate()))
        pcm = np.frombuffer(wf.readframes(wf.getnframes()), dtype=np.int16).reshape(-1, wf.getnchannels())
    x = np.zeros(SAMPLES, dtype=np.float32)
    n = min(SAMPLES, pcm.shape[0])
    x[:n] = pcm[:n].astype(np.float32).mean(axis=1) / 32768.0          # vggish_input.py:87-88
    return x


def band_hz(band):
    """Centre frequency of mel band 0..63 (64 HTK-mel bands from 125 to 7 500 Hz, mel_features.py:114-189)."""
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)                   # noqa: E731
    edges = np.linspace(mel(125.0), mel(7500.0), 66)
    return 700.0 * (np.exp(edges[band + 1] / 1127.0) - 1.0)


def main():
    args = sys.argv[1:]
    target = None
    if args and args[0] == "--target":
        target = int(args[1])
        args = args[2:]
    checkpoint = args.pop(0) if args and args[0].endswith(".pt") else None
    conf = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=1)
    clf = M.Ensemble("repeat", conf, [2, 1], torch.device("cuda"), precision="f32")
    sd = torch.load(checkpoint, map_location="cpu") if checkpoint else W.make_state_dict(6, W.ensemble_shapes((2, 1), False))
    clf.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    clf.cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        path = args[0] if args else synthetic(tmp)
        pcm = torch.as_tensor(read_16k(path)).cuda().reshape(1, SAMPLES)
    scores, examples, grad = clf.saliency_waveforms(pcm, target=target, times_input=True)
    k = int(scores[0].argmax()) if target is None else target
    print("%s: class %d (score %.3f)%s" % (os.path.basename(path), k, float(scores[0, k]), "" if target is None else " [asked for]"))
    cells = grad[0, :, 0].abs().flatten(1)                               # (10, 96 * 64): frame-major, band-minor
    total = float(cells.sum())
    for e in range(EXAMPLES):
        at = int(cells[e].argmax())
        frame, band = at // 64, at % 64
        print("  example %d  %5.2f s .. %5.2f s: largest |grad x input| %.3e at %5.2f s, mel band %2d (%4.0f Hz); share of the map %4.1f %%"
              % (e, 0.96 * e, 0.96 * (e + 1), float(cells[e, at]), 0.96 * e + 0.01 * frame, band, band_hz(band),
                 100.0 * float(cells[e].sum()) / total if total else 0.0))


if __name__ == "__main__":
    main()
