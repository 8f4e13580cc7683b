#!/usr/bin/env python3
"""Throughput of the HIP ResNet-50 trunk (cnn_type="resnet", just_bottlenecks=True): eval trunk in bf16 / f32 at 80 and
5 120 images, the frozen training step (TrainStep) at 8 and 64 bags, and -- as a yardstick only -- the same network built
from torch.nn.functional.conv2d in channels-last bf16 (MIOpen). Prints one JSON line.

    python scripts/resnet_bench.py [--quick] [--per-conv] [--dp-one-rank [--finetune]] [--finetune] [--from-waveforms]
                                   [--from-recordings]

--per-conv: instead, each distinct bf16 conv (and the stem) timed alone at 80 images against its own roofline.
--dp-one-rank: instead, the cost of the trunk's SyncBN on one GPU: the frozen bf16 step (eager) at 8 and 64 bags without a
process group and on a one-rank RCCL group with the collectives forced on (ops.Dist(always=True)), where each of the 53
BatchNorm2d layers runs sums -> all-reduce -> finish; the all-reduces are counted and timed from ops.Dist.trace.
--dp-one-rank --finetune: the same question for the trunk-FINETUNING bf16 step (cnn_trainable=True, 53 forward + 53 backward
SyncBN all-reduces and one flat gradient all-reduce per step): the step without a group (default graph mode: the yardstick, to
be read against profiles/resnet_finetune.json), without a group but eager, and on the one-rank RCCL group with the collectives
forced on (TrainStep(..., trunk_data_parallel=True); eager, as every data-parallel step), interleaved round by round in one
session on one device; writes profiles/resnet_dp_finetune_one_rank.json. More than one rank is not measured by this.
--finetune: instead, the trunk-finetuning step (cnn_trainable=True with the HIP trunk backward on, TrainStep, default graph
mode) in bf16 and f32 at 8 and 64 bags next to the frozen bf16 step, and torch autograd's forward + backward of the restated
ResNet-50 trunk (channels-last bf16, MIOpen, train mode) as the yardstick; writes profiles/resnet_finetune.json.
--from-waveforms: instead, the mel-dB front-end's share of the eval forward from audio: Ensemble.forward_clips on (bags, 88 200)
PCM against Ensemble.forward on the pre-made (bags, 10, 1, 224, 224) images, bf16 and f32 at 8 and 512 bags, the two timed
alternately round by round in one session; and the two front-end kernels timed alone by device events, with the bytes and
flops they need (counted from the shapes) over that time. Writes profiles/resnet_from_waveforms.json.
--from-recordings: instead, the step from decoded recordings to clips, on 4 s stereo int16 recordings at 44.1 kHz in host memory, bf16,
at 8 and 512 bags: Ensemble.forward_recordings, Ensemble.forward_clips on the ready clips, dataset.recordings_to_clips alone (host
packing, two copies, one launch), and the per-recording loop it replaces (frontend.as_device_mono(pcm16=True) -> frontend.resample ->
cut and zero fill, four launches per recording), medians of five rounds in which the four alternate; and the clips kernel alone by
device events with the bytes and flops it needs (counted from the shapes). Writes profiles/resnet_from_recordings.json.
"""

import importlib
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "audio-classification-using-a-deep-cnn-combined-with-multi-level-attention_amd"
M = importlib.import_module(PKG + ".model")
W = importlib.import_module(PKG + ".weights")
TR = importlib.import_module(PKG + ".train")
RN = importlib.import_module(PKG + ".resnet")

CONF = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
            first_cnn_layer_trainable=False, in_channels=3)


def timeit(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def miopen_trunk(ens, x):
    """Yardstick: the same trunk from F.conv2d / F.batch_norm in channels-last bf16 (eval mode)."""
    conv1, bn1, layers, _ = RN.parts(ens.cnn.cnn_model)
    cache = {}

    def w(c):
        if id(c) not in cache:
            cache[id(c)] = c.weight.detach().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        return cache[id(c)]

    def bn(t, m, relu):
        t = F.batch_norm(t, m.running_mean, m.running_var, m.weight.detach(), m.bias.detach(), False, 0.0, m.eps)
        return F.relu(t) if relu else t

    mean = torch.tensor([0.485, 0.456, 0.406], device=x.device).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=x.device).view(1, 3, 1, 1)

    def run():
        h = ((x.reshape(-1, 1, 224, 224).expand(-1, 3, -1, -1) - mean) / std).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        h = F.max_pool2d(bn(F.conv2d(h, w(conv1), stride=2, padding=3), bn1, True), 3, 2, 1)
        for layer in layers:
            for b in layer:
                o = bn(F.conv2d(h, w(b.conv1)), b.bn1, True)
                o = bn(F.conv2d(o, w(b.conv2), stride=b.stride, padding=1), b.bn2, True)
                o = bn(F.conv2d(o, w(b.conv3)), b.bn3, False)
                idn = bn(F.conv2d(h, w(b.downsample[0]), stride=b.stride), b.downsample[1], False) if b.downsample is not None else h
                h = F.relu(o + idn)
        return F.adaptive_avg_pool2d(h, 1).flatten(1).float()
    return run


def conv_rooflines(ens, n_img=80):
    """Each distinct bf16 conv of the trunk timed alone at n_img images, against max(FLOP / 2.5 PF, bytes / 8 TB/s)
    (bytes = input + weights + output once each); the stem against its own bound."""
    OPS = importlib.import_module(PKG + ".ops")
    dev = torch.device("cuda")
    conv1, bn1, layers, _ = RN.parts(ens.cnn.cnn_model)
    shapes, H = {}, 56
    for layer in layers:
        for b in layer:
            cin = b.conv1.in_channels
            for c, h, st in ((b.conv1, H, 1), (b.conv2, H, b.stride), (b.conv3, H // b.stride, 1)) + \
                    (((b.downsample[0], H, b.stride),) if b.downsample is not None else ()):
                key = (c.kernel_size[0], st, c.in_channels, c.out_channels, h)
                shapes[key] = shapes.get(key, 0) + 1
            H //= b.stride
    rows = []
    for (k, st, cin, cout, h), count in shapes.items():
        x = torch.randn(n_img, h, h, cin, device=dev).to(torch.bfloat16)
        w = OPS.rn_repack(torch.randn(cout, cin, k, k, device=dev) * 0.05, torch.bfloat16)
        ho = (h + 2 * (k // 2) - k) // st + 1
        t = timeit(lambda: OPS.rn_conv(x, w, st), 3, 20)
        flop = 2.0 * n_img * ho * ho * cout * k * k * cin
        byts = 2.0 * (n_img * h * h * cin + cout * k * k * cin + n_img * ho * ho * cout)
        bound = max(flop / 2.5e15, byts / 8e12)
        rows.append({"conv": "k%d s%d %d->%d @%d" % (k, st, cin, cout, h), "count": count, "us": round(t * 1e6, 1),
                     "roofline_us": round(bound * 1e6, 1), "fraction": round(bound / t, 3)})
    planes = torch.rand(n_img, 224, 224, device=dev)
    w1 = torch.randn(64, 3, 7, 7, device=dev) * 0.05
    t = timeit(lambda: OPS.rn_stem(planes, False, w1, torch.bfloat16), 3, 20)
    flop, byts = 2.0 * n_img * 112 * 112 * 64 * 147, 4.0 * n_img * 224 * 224 + 2.0 * n_img * 112 * 112 * 64
    bound = max(flop / 157e12, byts / 8e12)              # the stem runs on the f32 vector/FMA path: f32 MFMA peak as its bound
    rows.append({"conv": "stem k7 s2 3->64 @224", "count": 1, "us": round(t * 1e6, 1), "roofline_us": round(bound * 1e6, 1),
                 "fraction": round(bound / t, 3)})
    return rows


def dp_one_rank(sd):
    """See --dp-one-rank in the module docstring."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29517")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    ens = M.Ensemble("repeat", CONF, [2, 1], dev, precision="bf16")
    ens.load_state_dict(sd)
    ens.cuda()
    res = {"metric": "resnet50_frozen_step_dp_one_rank", "device": torch.cuda.get_device_name(0), "precision": "bf16",
           "just_bottlenecks": True}
    for bags in (8, 64):
        x = torch.rand(bags, 10, 1, 224, 224, device=dev)
        y = torch.arange(bags, device=dev) % 10
        for name, always in (("no_dist", "0"), ("dist_one_rank", "1")):
            os.environ["MLA_DIST_ALWAYS"] = always
            step = TR.TrainStep(ens, lr=1e-3, graph=False)
            assert step.dist.active == (always == "1")
            res["train_step_%d_bags_ms_%s" % (bags, name)] = round(timeit(lambda: step(x, y), 3, 10) * 1e3, 2)
            if always == "1":
                step.dist.trace, n = [], 5
                for _ in range(n):
                    step(x, y)
                torch.cuda.synchronize()
                rn = [t for t in step.dist.trace if t[0] == "syncbn_rn"]
                res["trunk_allreduces_per_step"] = len(rn) // n
                res["trunk_allreduce_bytes_per_step"] = sum(t[1] for t in rn) // n
                res["trunk_allreduce_ms_per_step_%d_bags" % bags] = round(sum(t[2].elapsed_time(t[3]) for t in rn) / n, 3)
                res["other_allreduces_per_step"] = (len(step.dist.trace) - len(rn)) // n
                step.dist.trace = None
                step.dist.close()
        res["dist_overhead_ms_%d_bags" % bags] = round(res["train_step_%d_bags_ms_dist_one_rank" % bags] -
                                                      res["train_step_%d_bags_ms_no_dist" % bags], 2)
    os.environ.pop("MLA_DIST_ALWAYS", None)
    print(json.dumps(res))
    dist.destroy_process_group()


def dp_finetune_one_rank(sd):
    """See --dp-one-rank --finetune in the module docstring."""
    import statistics
    import torch.distributed as dist
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def make(**kw):
        ens = M.Ensemble("repeat", dict(CONF, cnn_trainable=True), [2, 1], dev, precision="bf16", trunk_backward=True)
        ens.load_state_dict(sd)
        return TR.TrainStep(ens.cuda(), lr=1e-4, **kw)
    os.environ["MLA_DIST_ALWAYS"] = "0"
    steps = {"no_group": make(), "no_group_eager": make(graph=False)}          # built before any process group exists
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if "MASTER_PORT" not in os.environ:                                        # a free port: several users may share the host
        import socket
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(sock.getsockname()[1])
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    os.environ["MLA_DIST_ALWAYS"] = "1"
    steps["dist_one_rank"] = make(trunk_data_parallel=True)
    os.environ.pop("MLA_DIST_ALWAYS", None)
    assert steps["dist_one_rank"].dist.active and not steps["no_group"].dist.active and not steps["no_group_eager"].dist.active
    res = {"metric": "resnet50_finetune_step_dp_one_rank", "device": torch.cuda.get_device_name(0), "precision": "bf16",
           "just_bottlenecks": True, "optimizer": "adam lr 1e-4", "transport": steps["dist_one_rank"].dist.describe()["transport"],
           "rounds": 3, "steps_per_round": 5, "ranks_measured": 1}
    for bags in (8, 64):
        x = torch.rand(bags, 10, 1, 224, 224, device=dev)
        y = torch.arange(bags, device=dev) % 10
        times = {k: [] for k in steps}
        for step in steps.values():                                            # eager first step, graph capture, clocks
            timeit(lambda: step(x, y), 3, 1)
        for _ in range(res["rounds"]):
            for k, step in steps.items():
                times[k].append(timeit(lambda: step(x, y), 0, res["steps_per_round"]) * 1e3)
        for k, v in times.items():
            res["finetune_step_%d_bags_ms_%s" % (bags, k)] = round(statistics.median(v), 2)
            res["finetune_step_%d_bags_ms_%s_rounds" % (bags, k)] = [round(t, 2) for t in v]
        step = steps["dist_one_rank"]
        step.dist.trace, n = [], 5
        for _ in range(n):
            step(x, y)
        torch.cuda.synchronize()
        for tag in ("syncbn_rn", "syncbn_rn_bwd", "grad:flat"):
            sel = [t for t in step.dist.trace if t[0] == tag]
            key = tag.replace(":", "_")
            # counts and bytes do not depend on the number of bags (one key, written by both passes); the times do
            res["%s_allreduces_per_step" % key] = len(sel) // n
            res["%s_bytes_per_step" % key] = sum(t[1] for t in sel) // n
            res["%s_ms_per_step_%d_bags" % (key, bags)] = round(sum(t[2].elapsed_time(t[3]) for t in sel) / n, 3)
        res["other_allreduces_per_step"] = sum(t[0] not in ("syncbn_rn", "syncbn_rn_bwd", "grad:flat") for t in step.dist.trace) // n
        step.dist.trace = None
        res["peak_gb_%d_bags" % bags] = round(torch.cuda.max_memory_allocated() / 1e9, 2)     # the three steps together
        # two yardsticks: the eager no-group step isolates the collectives; the graphed one adds what eager launching costs
        res["dist_overhead_ms_%d_bags_vs_eager" % bags] = round(res["finetune_step_%d_bags_ms_dist_one_rank" % bags] -
                                                               res["finetune_step_%d_bags_ms_no_group_eager" % bags], 2)
        res["dist_overhead_ms_%d_bags_vs_graph" % bags] = round(res["finetune_step_%d_bags_ms_dist_one_rank" % bags] -
                                                               res["finetune_step_%d_bags_ms_no_group" % bags], 2)
    steps["dist_one_rank"].dist.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "resnet_dp_finetune_one_rank.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    dist.destroy_process_group()


def finetune(sd):
    """See --finetune in the module docstring."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import resnet50_restated as R
    dev = torch.device("cuda")
    res = {"metric": "resnet50_finetune_step", "device": torch.cuda.get_device_name(0), "just_bottlenecks": True, "optimizer": "adam lr 1e-4"}
    for bags in (8, 64):
        x = torch.rand(bags, 10, 1, 224, 224, device=dev)
        y = torch.arange(bags, device=dev) % 10
        for prec, trainable in (("bf16", False), ("bf16", True), ("f32", True)):
            ens = M.Ensemble("repeat", dict(CONF, cnn_trainable=trainable), [2, 1], dev, precision=prec, trunk_backward=True)
            ens.load_state_dict(sd)
            ens.cuda()
            step = TR.TrainStep(ens, lr=1e-4)
            torch.cuda.reset_peak_memory_stats()
            t = timeit(lambda: step(x, y), 3, 5)
            key = "%s_%s_%d_bags" % ("finetune" if trainable else "frozen", prec, bags)
            res[key + "_ms"] = round(t * 1e3, 2)
            res[key + "_peak_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
            del ens, step
            torch.cuda.empty_cache()
        m = R.CNN(True).cuda().to(torch.bfloat16).to(memory_format=torch.channels_last).train()
        for p in m.parameters():
            p.requires_grad_(True)
        xin = R.normalize_input(x, "repeat").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

        def torch_step():
            for p in m.parameters():
                p.grad = None
            m(xin).float().sum().backward()
        res["torch_autograd_trunk_fwd_bwd_bf16_%d_bags_ms" % bags] = round(timeit(torch_step, 3, 5) * 1e3, 2)
        del m, xin
        torch.cuda.empty_cache()
        res["finetune_over_frozen_bf16_%d_bags" % bags] = round(res["finetune_bf16_%d_bags_ms" % bags] / res["frozen_bf16_%d_bags_ms" % bags], 2)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "resnet_finetune.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def melspec_counts(bags, n=88200, hop=98, n_mels=224, n_images=10, width=224):
    """Bytes each front-end kernel must move and the flops of kernel 1, from the shapes alone."""
    frames = 1 + n // hop
    nnz = 2050                                                        # non-zero mel weights at (22 050 Hz, 224 bands)
    db_bytes = bags * (n * 4 + n_mels * frames * 4)                   # PCM in once, D out once
    img_bytes = bags * (n_mels * frames * 4 + n_images * n_mels * width * 4)
    # per frame: window 2048, five radix-4 stages of 256 butterflies (3 complex multiplies = 18 flops, 16 complex adds = 32 flops;
    # the first stage has no multiplies), the split to 1025 powers (about 17 flops each), 2 flops per mel weight
    flops = bags * frames * (2048 + 256 * (32 + 4 * 50) + 1025 * 17 + 2 * nnz)
    return db_bytes, img_bytes, flops


def from_waveforms(sd, quick):
    DS = importlib.import_module(PKG + ".dataset")
    OPS = importlib.import_module(PKG + ".ops")
    dev = torch.device("cuda")
    res = {"metric": "resnet50_from_waveforms", "device": torch.cuda.get_device_name(0), "rounds": 5}
    for prec in ("bf16", "f32"):
        ens = M.Ensemble("repeat", CONF, [2, 1], dev, precision=prec)
        ens.load_state_dict(sd)
        ens.cuda().eval()
        for bags in ((8,) if quick else (8, 512)):
            pcm = torch.rand(bags, 88200, device=dev) - 0.5           # timing only: the seeded statistics do not fit dB inputs
            iters = 3 if bags > 100 else 20
            with torch.no_grad():
                images = DS.clips_to_images(pcm)
                t_img, t_wav = [], []
                for _ in range(res["rounds"]):                         # alternate the two, so that drift hits both alike
                    t_img.append(timeit(lambda: ens(images), 1, iters))
                    t_wav.append(timeit(lambda: ens.forward_clips(pcm), 1, iters))
            t_img, t_wav = sorted(t_img)[len(t_img) // 2], sorted(t_wav)[len(t_wav) // 2]
            key = "%s_%d_bags" % (prec, bags)
            res[key + "_forward_images_ms"] = round(t_img * 1e3, 3)
            res[key + "_forward_clips_ms"] = round(t_wav * 1e3, 3)
            res[key + "_front_end_share"] = round((t_wav - t_img) / t_wav, 4)
        del ens
    for bags in ((8,) if quick else (8, 512)):                         # the two kernels alone, by device events
        pcm = torch.rand(bags, 88200, device=dev) - 0.5
        DS.clips_to_images(pcm)
        torch.cuda.synchronize()
        OPS.reserve_events(4 * 20)
        OPS.profile = []
        for _ in range(20):
            DS.clips_to_images(pcm)
        torch.cuda.synchronize()
        times = {}
        for name, e0, e1 in OPS.profile:
            times.setdefault(name, []).append(e0.elapsed_time(e1))
        OPS.profile = None
        db_bytes, img_bytes, flops = melspec_counts(bags)
        t_db, t_im = (sorted(times[k])[len(times[k]) // 2] * 1e-3 for k in ("melspec_db", "melspec_images"))
        res["kernels_%d_bags" % bags] = {
            "melspec_db_us": round(t_db * 1e6, 1), "melspec_db_GB_per_s": round(db_bytes / t_db / 1e9, 1),
            "melspec_db_GFLOP_per_s": round(flops / t_db / 1e9, 1),
            "melspec_images_us": round(t_im * 1e6, 1), "melspec_images_GB_per_s": round(img_bytes / t_im / 1e9, 1)}
    print(json.dumps(res))
    out = os.path.join(ROOT, "profiles", "resnet_from_waveforms.json")
    if not quick:
        with open(out, "w") as f:
            f.write(json.dumps(res) + "\n")


def from_recordings(sd, quick):
    import numpy as np
    DS = importlib.import_module(PKG + ".dataset")
    FE = importlib.import_module(PKG + ".frontend")
    OPS = importlib.import_module(PKG + ".ops")
    dev = torch.device("cuda")
    sr_in, n_in, n_out = 44100, 176400, 88200
    res = {"metric": "resnet50_from_recordings", "device": torch.cuda.get_device_name(0), "rounds": 5, "precision": "bf16",
           "recordings": "4 s stereo int16 at 44.1 kHz, host memory"}
    ens = M.Ensemble("repeat", CONF, [2, 1], dev, precision="bf16")
    ens.load_state_dict(sd)
    ens.cuda().eval()
    rng = np.random.default_rng(0)
    pool = [rng.integers(-16000, 16001, size=(n_in, 2)).astype(np.int16) for _ in range(8)]

    def loop(recs):
        """Today's calls, once per recording: mono mix (scaled), resampling, slice, copy into zeros."""
        out = torch.zeros((len(recs), n_out), dtype=torch.float32, device=dev)
        for i, x in enumerate(recs):
            y = FE.resample(FE.as_device_mono(x, pcm16=True), sr_in, 22050)
            k = min(y.shape[0], n_out)
            out[i, :k] = y[:k]
        return out

    for bags in ((8,) if quick else (8, 512)):
        recs = [pool[i % len(pool)] for i in range(bags)]
        iters = 3 if bags > 100 else 20
        with torch.no_grad():
            clips = DS.recordings_to_clips(recs, sr_in)
            res["%d_bags_batched_equals_loop" % bags] = bool(torch.equal(clips, loop(recs)))
            t = {"forward_recordings": [], "forward_clips": [], "recordings_to_clips": [], "per_recording_loop": []}
            for _ in range(res["rounds"]):                             # alternate, so that drift hits all alike
                t["forward_recordings"].append(timeit(lambda: ens.forward_recordings(recs, sr_in), 1, iters))
                t["forward_clips"].append(timeit(lambda: ens.forward_clips(clips), 1, iters))
                t["recordings_to_clips"].append(timeit(lambda: DS.recordings_to_clips(recs, sr_in), 1, iters))
                t["per_recording_loop"].append(timeit(lambda: loop(recs), 1, iters))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        for k, v in med.items():
            res["%d_bags_%s_ms" % (bags, k)] = round(v * 1e3, 3)
        res["%d_bags_step_share_of_forward_recordings" % bags] = round(med["recordings_to_clips"] / med["forward_recordings"], 4)
        res["%d_bags_loop_over_batched" % bags] = round(med["per_recording_loop"] / med["recordings_to_clips"], 2)
        # the kernel alone, by device events
        OPS.reserve_events(2 * 20)
        OPS.profile = []
        for _ in range(20):
            DS.recordings_to_clips(recs, sr_in)
        torch.cuda.synchronize()
        us = sorted(e0.elapsed_time(e1) * 1e3 for name, e0, e1 in OPS.profile if name == "clips_prepare")
        OPS.profile = None
        t_k = us[len(us) // 2] * 1e-6
        byts = bags * (n_in * 2 * 2 + n_out * 4)                       # PCM in once, clips out once (the 512 KB table stays in L2)
        flops = bags * n_out * (2 * 128 * 4 + 3)                       # two wings of 128 taps, two double fma each; the mix is staged
        res["%d_bags_clips_kernel_us" % bags] = round(t_k * 1e6, 1)
        res["%d_bags_clips_kernel_GB_per_s" % bags] = round(byts / t_k / 1e9, 1)
        res["%d_bags_clips_kernel_GFLOP_per_s_f64" % bags] = round(flops / t_k / 1e9, 1)
    print(json.dumps(res))
    if not quick:
        with open(os.path.join(ROOT, "profiles", "resnet_from_recordings.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


def main():
    quick = "--quick" in sys.argv
    dev = torch.device("cuda")
    sd = {k: torch.as_tensor(v) for k, v in W.make_state_dict(21, W.ensemble_shapes((2, 1), True, cnn_type="resnet")).items()}
    if "--dp-one-rank" in sys.argv:
        return dp_finetune_one_rank(sd) if "--finetune" in sys.argv else dp_one_rank(sd)
    if "--finetune" in sys.argv:
        return finetune(sd)
    if "--from-waveforms" in sys.argv:
        return from_waveforms(sd, quick)
    if "--from-recordings" in sys.argv:
        return from_recordings(sd, quick)
    if "--per-conv" in sys.argv:
        ens = M.Ensemble("repeat", CONF, [2, 1], dev, precision="bf16")
        ens.load_state_dict(sd)
        for r in conv_rooflines(ens.cuda().eval()):
            print(json.dumps(r))
        return
    res = {"metric": "resnet50_trunk", "device": torch.cuda.get_device_name(0)}
    for prec in ("bf16", "f32"):
        ens = M.Ensemble("repeat", CONF, [2, 1], dev, precision=prec)
        ens.load_state_dict(sd)
        ens.cuda().eval()
        for n_img in ((80,) if quick else (80, 5120)):
            x = torch.rand(n_img // 10, 10, 1, 224, 224, device=dev)
            with torch.no_grad():
                t = timeit(lambda: ens.cnn(ens.input(x)), 2, 5 if n_img > 1000 else 20)
            res["eval_%s_%d_img_per_s" % (prec, n_img)] = round(n_img / t, 1)
            res["eval_%s_%d_bags_per_s" % (prec, n_img)] = round(n_img / 10 / t, 1)
            if prec == "bf16":
                with torch.no_grad():
                    t = timeit(miopen_trunk(ens, x), 2, 5 if n_img > 1000 else 20)
                res["miopen_bf16_%d_img_per_s" % n_img] = round(n_img / t, 1)
        del ens
    ens = M.Ensemble("repeat", CONF, [2, 1], dev, precision="bf16")
    ens.load_state_dict(sd)
    ens.cuda()
    step = TR.TrainStep(ens, lr=1e-3)
    for bags in ((8,) if quick else (8, 64)):
        x = torch.rand(bags, 10, 1, 224, 224, device=dev)
        y = torch.arange(bags, device=dev) % 10
        t = timeit(lambda: step(x, y), 2, 5)
        res["train_step_bf16_%d_bags_ms" % bags] = round(t * 1e3, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
