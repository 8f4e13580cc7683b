#!/usr/bin/env python3
"""WAV files of any length -> one line per window with the top class: the VGGish branch scored over time. Every file is resampled to
16 kHz whole, scored in windows of four 0.96 s examples that start --hop-slots * 0.32 s apart (default 3: 0.96 s), and the CNN runs
once per distinct 0.96 s slot, however many windows share it (clf.score_timeline_audiofiles: two launches for the front-end, the CNN
in chunks, one gather, the head).

    python examples/wav_to_timeline.py [--hop-slots Q] [checkpoint.pt] a.wav b.wav ...

Without WAV files it writes two synthetic ones (a 20 s mono sweep at 8 kHz, 9 s of stereo tones at 44.1 kHz) to a temporary directory.
Without a checkpoint the weights are seeded, so the classes only show that the path runs."""

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


def synthetic(directory):
    t8, t44 = np.arange(20 * 8000) / 8000.0, np.arange(9 * 44100) / 44100.0
    files = {"sweep_8k_mono.wav": (8000, np.sin(2 * np.pi * (200 + 80 * t8) * t8)),
             "tones_44k_stereo.wav": (44100, np.stack([np.sin(2 * np.pi * 440 * t44), np.sin(2 * np.pi * 1320 * t44) * (t44 > 4)], axis=1))}
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
    hop_slots = 3
    if args and args[0] == "--hop-slots":
        hop_slots = int(args[1])
        args = args[2:]
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
            scores, index, starts = clf.score_timeline_audiofiles(paths, hop_slots=hop_slots)
    top = scores.argmax(dim=1).cpu().numpy()
    best = scores.max(dim=1).values.cpu().numpy()
    for w in range(scores.shape[0]):
        print("%s %7.2f s .. %7.2f s: class %d (%.3f)" % (os.path.basename(paths[index[w]]), starts[w], starts[w] + 3.855, top[w], best[w]))


if __name__ == "__main__":
    main()
