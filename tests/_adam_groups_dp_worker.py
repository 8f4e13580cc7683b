"""Worker of the 2-rank test of the grouped Adam step with gradient clipping (tests/test_adam_groups_gpu.py): each rank runs
TrainStep(optimizer=AdamW with two groups, max_grad_norm) on ITS half of every global batch (gloo, two ranks on one GPU, as
tests/_dp_worker.py). ``run`` is also what the test calls in its own process for the one-process twin on the global batch."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
PKG = "audio-classification-using-a-deep-cnn-combined-with-multi-level-attention_amd"

MAX_GRAD_NORM = 0.05


def run(steps, B, lo, hi, process_group):
    mk = importlib.import_module("make_golden")
    W = importlib.import_module(PKG + ".weights")
    M = importlib.import_module(PKG + ".model")
    TR = importlib.import_module(PKG + ".train")
    ens = M.Ensemble("repeat", dict(mk.CNN_CONF), [2, 1], torch.device("cuda"), precision="f32")
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(7, W.ensemble_shapes((2, 1), False)).items()})
    ens.cuda()
    named = [(n, p) for n, p in ens.named_parameters() if p.requires_grad and n.startswith("mla.")]
    is_w = lambda n, p: p.dim() >= 2 and ".norm" not in n                                          # noqa: E731
    opt = torch.optim.AdamW([dict(params=[p for n, p in named if is_w(n, p)], lr=1e-3, weight_decay=1e-2),
                             dict(params=[p for n, p in named if not is_w(n, p)], lr=3e-4, weight_decay=0.0)])
    step = TR.TrainStep(ens, optimizer=opt, max_grad_norm=MAX_GRAD_NORM, process_group=process_group)
    out = {"losses": [], "grad_norm": [], "clip_coef": []}
    for s in range(steps):
        x, y = mk.synth_bags(100 + s, B)
        masks = mk.make_masks(200 + s, [2, 1], B)
        for lvl, em in enumerate(ens.mla.embedded_mappings):
            for j, d in enumerate(em.dropouts):
                d.mask = masks["mla.embedded_mappings.%d.dropouts.%d" % (lvl, j)][lo:hi]
        loss, hits = step(x[lo:hi].cuda(), y[lo:hi].cuda())
        out["losses"].append(float(loss))
        out["grad_norm"].append(step.grad_norm.cpu().numpy()[0])
        out["clip_coef"].append(step.clip_coef.cpu().numpy()[0])
    res = {k: np.array(v) for k, v in out.items()}
    res.update({k: v.detach().cpu().numpy() for k, v in ens.state_dict().items() if k.startswith("mla.")})
    return res


def main():
    import torch.distributed as dist
    out_path, steps, B = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = run(steps, B, rank * B // world, (rank + 1) * B // world, None)
    np.savez(out_path + ".rank%d.npz" % rank, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
