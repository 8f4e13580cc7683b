#!/usr/bin/env python3
"""WAV files -> class scores with the ResNet branch: a ragged batch of recordings of any rate, channel count and encoding (8/16/24/32-bit
PCM, float32, float64) becomes the (B, 88 200) clips of 22 050 Hz PCM in one HIP launch, then mel-dB images, the ResNet-50 trunk and the attention head.

    python examples/wav_to_scores.py [--vggish] [checkpoint.pt] a.wav b.wav ...

--vggish scores the files with the VGGish branch instead: the reference's native dataset path (0.96 s log-mel examples in 4 slots,
no zero fill of the waveform, at most 4.8 s per file) in two launches, clf.forward_audiofiles_native(paths).
Without WAV files it writes two synthetic ones (mono 8 kHz, stereo 44.1 kHz) to a temporary directory. Without a checkpoint the
weights are seeded, so the scores only show that the path runs."""

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
dataset = importlib.import_module(PKG + ".dataset")


def synthetic(directory):
    t8, t44 = np.arange(3 * 8000) / 8000.0, np.arange(4 * 44100) / 44100.0
    files = {"siren_8k_mono.wav": (8000, np.sin(2 * np.pi * (400 + 200 * np.sin(2 * np.pi * t8)) * t8)),
             "tones_44k_stereo.wav": (44100, np.stack([np.sin(2 * np.pi * 440 * t44), np.sin(2 * np.pi * 1320 * t44)], axis=1))}
    paths = []
    for name, (rate, x) in files.items():
        pcm = (x * 12000).astype(np.int16)
        with wave.open(os.path.join(directory, name), "wb") as wf:
            wf.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1])
            wf.setsampwidth(2)
            wf.setframerate(rate)
            wf.writeframes(pcm.tobytes())
        paths.append(os.path.join(directory, name))
    return paths


def main():
    args = sys.argv[1:]
    if args and args[0] == "--vggish":
        return main_vggish(args[1:])
    checkpoint = args.pop(0) if args and args[0].endswith(".pt") else None
    conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    clf = M.Ensemble("repeat", conf, [2, 1], torch.device("cuda"), precision="bf16")
    if checkpoint:
        clf.load_state_dict(torch.load(checkpoint, map_location="cpu"))
    else:
        sd = W.make_state_dict(11, W.ensemble_shapes((2, 1), True, cnn_type="resnet"))
        clf.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    clf.cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        paths = args or synthetic(tmp)
        with torch.no_grad():
            if not checkpoint:
                # seeded running statistics describe unit-scale inputs, not dB images: the eval-mode attention would underflow to
                # 0 / 0. A trained checkpoint's statistics describe its data; here thirty train-mode passes stand in for that.
                images = dataset.clips_to_images(dataset.audiofiles_to_clips(paths))
                clf.train()
                for _ in range(30):
                    clf(images)
                clf.eval()
            clips = dataset.audiofiles_to_clips(paths)               # (B, 88200) float32 on the GPU, decoded in one launch
            scores = clf.forward_clips(clips)                        # the same as clf.forward_audiofiles(paths)
    for path, clip, row in zip(paths, clips, scores):
        print("%s: %d of 88200 samples non-zero, scores %s" % (os.path.basename(path), int((clip != 0).sum()),
                                                                np.array2string(row.float().cpu().numpy(), precision=3)))


def main_vggish(args):
    checkpoint = args.pop(0) if args and args[0].endswith(".pt") else None
    conf = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=1)
    clf = M.Ensemble("repeat", conf, [2, 1], torch.device("cuda"), precision="bf16")
    sd = torch.load(checkpoint, map_location="cpu") if checkpoint else W.make_state_dict(6, W.ensemble_shapes((2, 1), False))
    clf.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    clf.cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        paths = args or synthetic(tmp)
        with torch.no_grad():
            frames = dataset.audiofiles_to_frames(paths)             # (B, 10, 1, 64, 96) float32 on the GPU, two launches
            scores = clf.forward_audiofiles_native(paths)            # the same bags, written in bf16, through the CNN and the head
    for path, bag, row in zip(paths, frames, scores):
        print("%s: %d of 4 slots filled, scores %s" % (os.path.basename(path), int((bag[::3, 0] != 0).any(dim=2).any(dim=1).sum()),
                                                       np.array2string(row.float().cpu().numpy(), precision=3)))


if __name__ == "__main__":
    main()
