"""The cross-entropy with options (mla_cross_entropy_den + mla_cross_entropy_opts: denominator, one wavefront per row, finish)
against the plain kernel (mla_cross_entropy: one workgroup, a serial K loop per row) on the same scores, and what the criterion
costs the training step: device-event times in one process, the variants alternated window by window (a difference is judged by
the spread of the windows).

  kernels  512 x 10, 512 x 527, 5 120 x 10:  old | new with plain options | new with weights, smoothing 0.1 and ignored rows
  step     the frozen-CNN step at 512 bags, eager, without and with criterion=CrossEntropyLoss(weight, label_smoothing=0.1)
  replay   the 8-bag step as a HIP graph replay, without and with it

Asserts the one requirement: at 512 x 527 the new sequence is faster than mla_cross_entropy measured in the same run.
usage: loss_bench.py [--windows 7] [--iters 200] [--step-iters 10] [--no-step] [--out file.json]"""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
import torch

PKG = "audio-classification-using-a-deep-cnn-combined-with-multi-level-attention_amd"
ops = importlib.import_module(PKG + ".ops")
W = importlib.import_module(PKG + ".weights")


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters                    # microseconds


def alternate(variants, windows, iters):
    for fn in variants.values():
        window(fn, 3)
    times = {k: [] for k in variants}
    for _ in range(windows):
        for k, fn in variants.items():
            times[k].append(window(fn, iters))
    out = {}
    for k, ts in times.items():
        ts = sorted(ts)
        out[k] = {"us_median": ts[len(ts) // 2], "us_min": ts[0], "us_max": ts[-1]}
    return out


def kernels(rows, K, windows, iters):
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(W.uniform(11, 1, rows * K, lo=0.0, hi=1.0)).reshape(rows, K).to(dev)      # the head's scores are sigmoid outputs
    y = torch.from_numpy(W.bits24(11, 2, rows) % K).to(dev)
    y_ign = y.clone()
    y_ign[::4] = -100
    w = torch.linspace(0.5, 2.0, K, device=dev)
    res = alternate({
        "old": lambda: ops.cross_entropy(x, y, 1.0 / rows),
        "new_plain": lambda: ops.cross_entropy_opts(x, y),
        "new_options": lambda: ops.cross_entropy_opts(x, y_ign, w, -100, 0.1, "mean"),
    }, windows, iters)
    res.update(rows=rows, K=K, iters_per_window=iters, windows=windows, old_over_new_plain=res["old"]["us_median"] / res["new_plain"]["us_median"])
    return res


def steps(B, graph, windows, iters):
    mk = importlib.import_module("make_golden")
    M = importlib.import_module(PKG + ".model")
    TR = importlib.import_module(PKG + ".train")
    x, y = mk.synth_bags(3, B)
    x, y = x.cuda(), y.cuda()
    y_ign = y.clone()
    y_ign[::4] = -100
    variants = {}
    for name, crit in (("plain", None), ("criterion", torch.nn.CrossEntropyLoss(weight=torch.linspace(0.5, 2.0, 10), label_smoothing=0.1))):
        ens = M.Ensemble("repeat", dict(mk.CNN_CONF), [2, 1], torch.device("cuda"))
        ens.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(7, W.ensemble_shapes((2, 1), False)).items()})
        ens.cuda()
        step = TR.TrainStep(ens, lr=1e-3, graph=graph, criterion=crit)
        labels = y if crit is None else y_ign
        for _ in range(3):                                        # the first step sizes the scratch, the second records the graph
            step(x, labels)
        assert (step._graph is not None) == graph
        variants[name] = (lambda s=step, l=labels: s(x, l))
    res = alternate(variants, windows, iters)
    res.update(bags=B, graph=graph, iters_per_window=iters, windows=windows,
               criterion_minus_plain_us=res["criterion"]["us_median"] - res["plain"]["us_median"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    results = {"kernels": [], "steps": []}
    for rows, K in ((512, 10), (512, 527), (5120, 10)):
        results["kernels"].append(kernels(rows, K, a.windows, a.iters))
        print(json.dumps(results["kernels"][-1]))
    if not a.no_step:
        for B, graph, iters in ((512, False, a.step_iters), (8, True, a.step_iters * 10)):
            results["steps"].append(steps(B, graph, a.windows, iters))
            print(json.dumps(results["steps"][-1]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    wide = results["kernels"][1]
    assert wide["new_plain"]["us_median"] < wide["old"]["us_median"] and wide["new_options"]["us_median"] < wide["old"]["us_median"], \
        "at 512 x 527 the new sequence must be faster than mla_cross_entropy"


if __name__ == "__main__":
    main()
