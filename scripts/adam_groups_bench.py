"""The grouped Adam step (mla_adam_grouped_step) against the one-group kernel (mla_adam_step) on the same flat buffers, and
mla_grad_norm: device-event times, bytes per parameter and TB/s against the ~6.3 TB/s streaming ceiling.

Variants, alternated window by window in one process (the spread of the old kernel's own windows is what a difference is
judged by):  old      mla_adam_step
             plain    the grouped step with one group, no decay, no amsgrad, no clip pointer (the old kernel's bits)
             full     three interleaved groups (L2 decay | decoupled decay | amsgrad) with the clip coefficient
             norm     mla_grad_norm alone
Sizes: the head's flat size and the full VGGish finetune set (every tensor padded to 4 floats). Bytes per parameter: 28 for Adam
(read p, g, m, v; write p, m, v), 36 where amsgrad also reads and writes vmax (a third of `full`: 30.7 on average), 4 for the norm.
usage: adam_groups_bench.py [--windows 7] [--iters 50] [--out file.json]"""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

PKG = "audio-classification-using-a-deep-cnn-combined-with-multi-level-attention_amd"
ops = importlib.import_module(PKG + ".ops")
W = importlib.import_module(PKG + ".weights")

PLAIN = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, amsgrad=False)
FULL = [dict(PLAIN, weight_decay=1e-2), dict(PLAIN, lr=3e-4, weight_decay=5e-2, decoupled=True), dict(PLAIN, lr=1e-4, amsgrad=True)]


def layouts():
    """{name: [numel per tensor]} in named_parameters() order: the head alone, and the whole VGGish ensemble (fcf left out)."""
    shapes = W.ensemble_shapes((2, 1), False)
    skip = ("running_", "num_batches", ".fcf.")
    params = [(n, int(torch.Size(s).numel())) for n, s in shapes.items() if not any(k in n for k in skip)]
    return {"head": [k for n, k in params if n.startswith("mla.")], "vggish_finetune": [k for _, k in params]}


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda", 0)
    results = []
    for name, numels in layouts().items():
        one = ops.adam_groups_table(numels, [0] * len(numels), 1)
        three = ops.adam_groups_table(numels, [i % 3 for i in range(len(numels))], 3)
        n = one["total"]
        p = torch.from_numpy(W.uniform(3, 1, n, lo=-1.0, hi=1.0)).to(dev)
        g = torch.from_numpy(W.uniform(3, 2, n, lo=-1e-2, hi=1e-2)).to(dev)
        m, v, vmax = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
        rows1, rows3 = torch.zeros(8, device=dev), torch.zeros(24, device=dev)
        ops.adam_groups_prepare(rows1, [PLAIN], 10)
        ops.adam_groups_prepare(rows3, FULL, 10)
        t1, t3 = one["table"].to(dev), three["table"].to(dev)
        clip = ops.grad_norm(g, 1.0)
        ws = torch.zeros(1024, dtype=torch.float64, device=dev)
        variants = {
            "old": lambda: ops.adam_step(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 10),
            "plain": lambda: ops.adam_grouped_step(p, g, m, v, None, t1, one["runs"], one["pads"], rows1, 1),
            "full": lambda: ops.adam_grouped_step(p, g, m, v, vmax, t3, three["runs"], three["pads"], rows3, 3, clip[1:2]),
            "norm": lambda: ops.grad_norm(g, 1.0, out=clip, workspace=ws),
        }
        iters = a.iters if n > 10 ** 7 else a.iters * 20         # the head's step is microseconds: time enough of them
        for fn in variants.values():                                # warm-up: code objects, caches
            window(fn, 5)
        times = {k: [] for k in variants}
        for _ in range(a.windows):                                  # alternate the variants window by window
            for k, fn in variants.items():
                times[k].append(window(fn, iters))
        bytes_per = {"old": 28.0, "plain": 28.0, "full": 28.0 + 8.0 / 3.0, "norm": 4.0}
        row = {"layout": name, "n_padded": n, "tensors": len(numels), "runs_full": three["runs"], "iters_per_window": iters, "windows": a.windows}
        for k, ts in times.items():
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            row[k] = {"ms_median": med, "ms_min": ts[0], "ms_max": ts[-1], "spread_rel": (ts[-1] - ts[0]) / med,
                      "bytes_per_param": bytes_per[k], "TB_per_s": bytes_per[k] * n / med / 1e9, "share_of_6.3TBps": bytes_per[k] * n / med / 1e9 / 6.3}
        row["plain_over_old"] = row["plain"]["ms_median"] / row["old"]["ms_median"]
        row["full_over_plain"] = row["full"]["ms_median"] / row["plain"]["ms_median"]
        results.append(row)
        print(json.dumps(row))
        del p, g, m, v, vmax
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
