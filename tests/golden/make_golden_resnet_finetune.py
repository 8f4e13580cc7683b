#!/usr/bin/env python3
"""Generates tests/golden/resnet_finetune.npz by running the REFERENCE's own Ensemble with gradients into the ResNet-50 trunk
(build container only; the reference tree is not on the GPU machines).

Usage (from the repo root, in the container that has the reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_resnet_finetune.py

As make_golden_resnet.py: torchvision's resnet50 is stubbed by the float64 restatement (tests/resnet50_restated.py), dropout
masks are injected, everything runs in float64. Two runs of three literal steps (train.py:124-138) with
torch.optim.Adam(lr=1e-4) over the trainable parameters (train.py:283-303, the finetune workflow of train.py:96-97 / :370)
on 2 bags:
  a  cnn_trainable=True,              just_bottlenecks=True,  input "repeat"  (the whole trunk trains)
  b  first_cnn_layer_trainable=True,  just_bottlenecks=False, input "single"  (conv1 and the fc train; the stem's zero channels)
Stored per run: the three losses, the step-1 scores, and for every parameter (named_parameters() order, `names`) the step-1
gradient norm (NaN where .grad stays None), 32 step-1 gradient values and the initial / final (after step 3) values at 32
seeded flat indices (stored with them, -1 past a smaller tensor); 32 sampled values of every final running statistic.
"""

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden_resnet import CONF, SEED, W, images, import_reference, labels  # noqa: E402
from make_golden import install_masks, make_masks  # noqa: E402

RUNS = {"a": dict(conf="repeat", jb=True, cnn_trainable=True, first_cnn_layer_trainable=False),
        "b": dict(conf="single", jb=False, cnn_trainable=False, first_cnn_layer_trainable=True)}
LR = 1e-4
NS = 32


def sample_idx(name, numel):
    rng = np.random.default_rng(W.stream_id("finetune_idx/" + name))
    return np.sort(rng.choice(numel, size=min(NS, numel), replace=False)).astype(np.int64)


def build(ref_model, run):
    cnn_conf = dict(CONF, just_bottlenecks=run["jb"], cnn_trainable=run["cnn_trainable"],
                    first_cnn_layer_trainable=run["first_cnn_layer_trainable"])
    ens = ref_model.Ensemble(run["conf"], cnn_conf, [2, 1], torch.device("cpu"))
    sd = W.make_state_dict(SEED, W.ensemble_shapes((2, 1), run["jb"], cnn_type="resnet", num_classes=10))
    ens.load_state_dict({k: torch.as_tensor(v).double() if v.dtype != np.int64 else torch.as_tensor(v) for k, v in sd.items()},
                        strict=True)
    return ens


def gen_run(ref_model, tag, run):
    """Arrays of one run; per-parameter samples are stacked (P, 32) in named_parameters() order, idx -1 past a small tensor."""
    ens = build(ref_model, run)
    named = list(ens.named_parameters())
    P = len(named)
    idx = np.full((P, NS), -1, dtype=np.int64)
    for r, (n, p) in enumerate(named):
        i = sample_idx(n, p.numel())
        idx[r, :len(i)] = i
    take = lambda t, r: np.where(idx[r] >= 0, t.detach().reshape(-1).numpy()[np.maximum(idx[r], 0)], 0.0)   # noqa: E731
    init = np.stack([take(p, r) for r, (_, p) in enumerate(named)])
    grad, gnorm = np.zeros((P, NS)), np.full(P, np.nan)
    params = [p for p in ens.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=LR)
    crit = torch.nn.CrossEntropyLoss()
    ens.train()
    losses = []
    for s in range(3):
        install_masks(ens.mla, make_masks(200 + s, [2, 1], 2))
        opt.zero_grad()
        out = ens(images(10 + s, 2))
        loss = crit(out, labels(2, s))
        loss.backward()
        if s == 0:
            scores1 = out.detach().numpy()
            for r, (n, p) in enumerate(named):
                if p.grad is not None:
                    gnorm[r] = float(p.grad.norm())
                    grad[r] = take(p.grad, r)
        opt.step()
        losses.append(loss.item())
    final = np.stack([take(p, r) for r, (_, p) in enumerate(named)])
    stats = [(k, v) for k, v in ens.cnn.state_dict().items() if k.endswith(("running_mean", "running_var"))]
    stat_idx = np.stack([sample_idx(k, v.numel()) for k, v in stats])
    stat = np.stack([v.reshape(-1).numpy()[i] for (_, v), i in zip(stats, stat_idx)])
    f32 = lambda a: a.astype(np.float32)      # noqa: E731
    return {tag + "/names": np.array([n for n, _ in named]), tag + "/idx": idx.astype(np.int32), tag + "/init": f32(init),
            tag + "/grad": f32(grad), tag + "/gnorm": gnorm, tag + "/final": f32(final), tag + "/losses": np.array(losses),
            tag + "/scores1": scores1, tag + "/stat_names": np.array([k for k, _ in stats]), tag + "/stat_idx": stat_idx.astype(np.int32),
            tag + "/stat": f32(stat)}


def main():
    torch.set_num_threads(os.cpu_count() or 1)
    torch.set_default_dtype(torch.float64)
    ref_model = import_reference()
    g = {}
    for tag, run in RUNS.items():
        g.update(gen_run(ref_model, tag, run))
    path = os.path.join(HERE, "resnet_finetune.npz")
    np.savez_compressed(path, **g)
    print("resnet_finetune.npz %d arrays %.1f KB" % (len(g), os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
