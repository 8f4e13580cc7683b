#!/usr/bin/env python3
"""The head beyond 16 classes measured on one device. Prints one JSON line and writes
profiles/wide_head.json (or the file given with --out).

    python scripts/wide_head_bench.py [--quick] [--out FILE]

Kernels, by device events, median of 50 launches after warm-up, the whole measurement five times (the figure is the median of
the five medians, `spread` their (max - min) / median):
  attention_pool (save=True) and attention_pool_bwd at 512 and 5 120 bags x T = 10 x K = 527, in microseconds and as a fraction of
  8 TB/s over the bytes each must move (forward: z read once, att and cla written, y written; backward: att, cla, dy read, du_v and
  du_f written). Yardstick: the oracle's torch-eager expression of the same step on the same device (softmax / sigmoid of the two
  BatchNorm outputs, the pooling; backward through torch autograd of that expression).
  cross_entropy at 512 x 527 (one block, a serial K loop per row: left as it is).
Training step: frozen VGGish in bf16, 512 bags, Ensemble(classes=527) against the default classes=10, the two alternating step by
step in one process (eager and as the HIP graph), median of five rounds of 10 steps.
--quick: 8 bags, one repeat, nothing written.
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
TR = importlib.import_module(PKG + ".train")
OPS = importlib.import_module(PKG + ".ops")

CONF = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False, cnn_trainable=False,
            first_cnn_layer_trainable=False, in_channels=1)
T, K = 10, 527
HBM = 8.0e12


def median(xs):
    return sorted(xs)[len(xs) // 2]


def event_us(fn, launches):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for e0, e1 in evs:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return median([e0.elapsed_time(e1) * 1e3 for e0, e1 in evs])


def repeated(fn, repeats, launches):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    meds = [event_us(fn, launches) for _ in range(repeats)]
    m = median(meds)
    return m, (max(meds) - min(meds)) / m


def pooling(bags, repeats, launches):
    g = torch.Generator(device="cuda").manual_seed(bags)
    z = torch.randn(bags * T, K, device="cuda", generator=g)
    bn = lambda: [torch.randn(T, device="cuda", generator=g) * 0.1, torch.rand(T, device="cuda", generator=g) + 0.5,          # noqa: E731
                  torch.rand(T, device="cuda", generator=g) + 0.5, torch.randn(T, device="cuda", generator=g) * 0.1]
    nv, nf = bn(), bn()
    y = torch.empty(bags, 2 * K, device="cuda")[:, :K]
    dy = torch.randn(bags, K, device="cuda", generator=g)
    att, cla = OPS.attention_pool(z, bags, T, K, nv, nf, y, save=True)
    out = {}
    fwd_bytes = 4 * (3 * bags * T * K + bags * K)
    bwd_bytes = 4 * (4 * bags * T * K + bags * K)
    for name, fn, nbytes in (("attention_pool", lambda: OPS.attention_pool(z, bags, T, K, nv, nf, y, save=True), fwd_bytes),
                             ("attention_pool_bwd", lambda: OPS.attention_pool_bwd(dy, att, cla, bags, T, K), bwd_bytes)):
        us, spread = repeated(fn, repeats, launches)
        out[name] = {"us": round(us, 2), "spread": round(spread, 3), "bytes": nbytes, "of_8TBs": round(nbytes / (us * 1e-6) / HBM, 4)}

    def eager_fwd(leaf=False):
        z3 = z.reshape(bags, T, K)
        u_v = (z3 - nv[0].view(1, T, 1)) * torch.rsqrt(nv[1].view(1, T, 1) + 1e-5) * nv[2].view(1, T, 1) + nv[3].view(1, T, 1)
        u_f = (z3 - nf[0].view(1, T, 1)) * torch.rsqrt(nf[1].view(1, T, 1) + 1e-5) * nf[2].view(1, T, 1) + nf[3].view(1, T, 1)
        if leaf:
            u_v, u_f = u_v.detach().requires_grad_(True), u_f.detach().requires_grad_(True)
        a, c = torch.softmax(u_v, dim=2), torch.sigmoid(u_f)
        return u_v, u_f, (c * (a / a.sum(dim=1, keepdim=True))).sum(dim=1)

    us, spread = repeated(lambda: eager_fwd(), repeats, launches)
    out["torch_eager_forward"] = {"us": round(us, 2), "spread": round(spread, 3)}

    def eager_bwd():
        u_v, u_f, yy = eager_fwd(leaf=True)
        torch.autograd.grad(yy, (u_v, u_f), dy)
    us2, spread2 = repeated(eager_bwd, repeats, launches)
    out["torch_eager_forward_plus_backward"] = {"us": round(us2, 2), "spread": round(spread2, 3)}
    return out


def cross_entropy(rows, repeats, launches):
    g = torch.Generator(device="cuda").manual_seed(7)
    scores = torch.rand(rows, K, device="cuda", generator=g)
    labels = torch.randint(0, K, (rows,), device="cuda", generator=g)
    us, spread = repeated(lambda: OPS.cross_entropy(scores, labels, 1.0 / rows), repeats, launches)
    return {"us": round(us, 2), "spread": round(spread, 3)}


def train_steps(bags, rounds, steps):
    res = {}
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(bags, 10, 1, 96, 64, generator=g) * 6.0 - 1.4).cuda()
    models = {}
    for graph in (False, True):
        for classes in (10, K):
            torch.manual_seed(5)
            ens = M.Ensemble("repeat", dict(CONF), [2, 1], torch.device("cuda"), precision="bf16", classes=classes).cuda()
            y = torch.randint(0, classes, (bags,), generator=g).cuda()
            step = TR.TrainStep(ens, lr=1e-3, graph=graph)
            for _ in range(3):
                step(x, y)
            models[(graph, classes)] = (step, y)
    torch.cuda.synchronize()
    for graph in (False, True):
        times = {10: [], K: []}
        for _ in range(rounds):
            for classes in (10, K):
                step, y = models[(graph, classes)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(x, y)
                torch.cuda.synchronize()
                times[classes].append((time.perf_counter() - t0) / steps * 1e3)
        for classes in (10, K):
            m = median(times[classes])
            res["%s_classes_%d_ms" % ("graph" if graph else "eager", classes)] = round(m, 3)
            res["%s_classes_%d_spread" % ("graph" if graph else "eager", classes)] = round((max(times[classes]) - min(times[classes])) / m, 3)
    return res


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "wide_head.json")
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    repeats, launches = (1, 5) if quick else (5, 50)
    res = {"device": torch.cuda.get_device_name(0), "T": T, "K": K, "pooling": {}}
    for bags in ((8,) if quick else (512, 5120)):
        res["pooling"][str(bags)] = pooling(bags, repeats, launches)
    res["cross_entropy_512x527"] = cross_entropy(8 if quick else 512, repeats, launches)
    res["frozen_train_step_bf16"] = dict(bags=8 if quick else 512, **train_steps(8 if quick else 512, 1 if quick else 5, 2 if quick else 10))
    print(json.dumps(res))
    if not quick:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
