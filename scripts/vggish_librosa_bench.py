#!/usr/bin/env python3
"""The VGGish branch's librosa path (HTK mel-dB bags) measured on one device. Prints one JSON line and
writes profiles/vggish_librosa.json.

    python scripts/vggish_librosa_bench.py [--quick]

Kernels: melspec_nopad_db_kernel and the clip-and-gather kernel timed alone by device events at 8 and 512 clips of 64 000
samples, median of 20 launches after warm-up. Comparator: the centred kernel of the ResNet branch at the same band count and hop
on the same rows, frontend.melspectrogram_db(pcm, 16000, 64, 160, top_db=None) (melspec_db_kernel: 401 frames against 388), the two
alternating launch by launch in one process; both are reported in microseconds per frame. The whole measurement is repeated five
times: the reported figure is the median of the five medians and `spread` their (max - min) / median, which is what the ratio of
the two kernels can be trusted to.
Share of the forward: Ensemble.forward_clips_librosa on PCM against Ensemble.forward on the pre-made bags (in the compute dtype),
bf16 and f32 at 8 and 512 bags, alternating, median of five rounds -- as scripts/resnet_bench.py --from-waveforms does.
--quick: 8 clips only, nothing written.
"""

import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "audio-classification-using-a-deep-cnn-combined-with-multi-level-attention_amd"
M = importlib.import_module(PKG + ".model")
W = importlib.import_module(PKG + ".weights")
DS = importlib.import_module(PKG + ".dataset")
FE = importlib.import_module(PKG + ".frontend")
OPS = importlib.import_module(PKG + ".ops")

CONF = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False, cnn_trainable=False,
            first_cnn_layer_trainable=False, in_channels=1)
N, HOP, BANDS, SR = DS.SAMPLES_NUM_VGGISH_LIBROSA, DS.LIBROSA_HOP, DS.LIBROSA_N_MELS, DS.SR_VGGISH
REPEATS, LAUNCHES = 5, 20


def timeit(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def median(xs):
    return sorted(xs)[len(xs) // 2]


def kernels(clips):
    """Median-of-20 device-event times (us) of the three kernels, the new pair and the comparator alternating, five times over."""
    pcm = torch.rand(clips, N, device="cuda") - 0.5
    new = lambda: DS.clips_to_frames_librosa(pcm)                                      # noqa: E731
    old = lambda: FE.melspec_db_unclipped(pcm, SR, BANDS, HOP)                         # noqa: E731
    for _ in range(3):
        new(), old()
    torch.cuda.synchronize()
    meds = {"melspec_nopad_db": [], "melspec_nopad_bags": [], "melspec_db": []}
    for _ in range(REPEATS):
        OPS.reserve_events(2 * 3 * LAUNCHES)
        OPS.profile = []
        for _ in range(LAUNCHES):
            new(), old()
        torch.cuda.synchronize()
        times = {}
        for name, e0, e1 in OPS.profile:
            times.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
        OPS.profile = None
        for k in meds:
            meds[k].append(median(times[k]))
    f_new, f_old = FE.melspec_frames_librosa(N, HOP), FE.melspec_frames(N, HOP)
    out = {"frames_new": f_new, "frames_comparator": f_old}
    for k, frames in (("melspec_nopad_db", f_new), ("melspec_nopad_bags", f_new), ("melspec_db", f_old)):
        m = median(meds[k])
        out[k + "_us"] = round(m, 1)
        out[k + "_us_per_frame"] = round(m / (clips * frames), 5)
        out[k + "_spread"] = round((max(meds[k]) - min(meds[k])) / m, 4)
    out["nopad_db_over_comparator_per_frame"] = round(out["melspec_nopad_db_us"] / f_new / (out["melspec_db_us"] / f_old), 4)
    return out


def share(sd, quick):
    res = {}
    for prec in ("bf16", "f32"):
        ens = M.Ensemble("repeat", CONF, [2, 1], torch.device("cuda"), precision=prec)
        ens.load_state_dict(sd)
        ens.cuda().eval()
        dtype = torch.bfloat16 if prec == "bf16" else torch.float32
        for bags in ((8,) if quick else (8, 512)):
            pcm = torch.rand(bags, N, device="cuda") - 0.5                             # timing only: the seeded statistics do not fit dB inputs
            iters = 5 if bags > 100 else 20
            with torch.no_grad():
                ready = DS.clips_to_frames_librosa(pcm, dtype)
                t_bags, t_pcm = [], []
                for _ in range(5):                                                     # alternate the two, so that drift hits both alike
                    t_bags.append(timeit(lambda: ens(ready), 1, iters))
                    t_pcm.append(timeit(lambda: ens.forward_clips_librosa(pcm), 1, iters))
            t_bags, t_pcm = median(t_bags), median(t_pcm)
            key = "%s_%d_bags" % (prec, bags)
            res[key + "_forward_bags_ms"] = round(t_bags * 1e3, 3)
            res[key + "_forward_clips_librosa_ms"] = round(t_pcm * 1e3, 3)
            res[key + "_front_end_share"] = round((t_pcm - t_bags) / t_pcm, 4)
        del ens
    return res


def main():
    quick = "--quick" in sys.argv
    assert torch.cuda.is_available(), "needs cuda:0"
    res = {"metric": "vggish_librosa_front_end", "device": torch.cuda.get_device_name(0), "launches": LAUNCHES, "repeats": REPEATS}
    for clips in ((8,) if quick else (8, 512)):
        res["kernels_%d_clips" % clips] = kernels(clips)
    sd = {k: torch.as_tensor(v) for k, v in W.make_state_dict(6, W.ensemble_shapes((2, 1), False)).items()}
    res.update(share(sd, quick))
    print(json.dumps(res))
    if not quick:
        with open(os.path.join(ROOT, "profiles", "vggish_librosa.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
