"""Worker of the 2-rank test of the multi-label training step (tests/test_bce_gpu.py): each rank runs
TrainStep(criterion=BCELoss(weight)) on ITS half of every global batch (gloo, two ranks on one GPU, as tests/_ce_opts_dp_worker.py).
The mean's scale is 1 / (global batch x classes) on both ranks, so the summed losses are the one-process mean. ``run`` is also
what the test calls in its own process for the one-process twin; ``targets`` makes the multi-hot labels every step test uses."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
PKG = "audio-classification-using-a-deep-cnn-combined-with-multi-level-attention_amd"


def criterion(**kw):
    return torch.nn.BCELoss(weight=torch.linspace(0.5, 2.0, 10), **kw)


def targets(seed, B, K=10, soft=4):
    """(B, K) float32 multi-hot targets, three in ten set, every row with at least one tag, and `soft` entries inside (0, 1)."""
    rng = np.random.default_rng(9000 + seed)
    y = (rng.uniform(0, 1, (B, K)) < 0.3).astype(np.float32)
    y[np.arange(B), rng.integers(0, K, B)] = 1.0
    for _ in range(soft):
        y[rng.integers(0, B), rng.integers(0, K)] = np.float32(rng.uniform(0.1, 0.9))
    return torch.from_numpy(y)


def run(steps, B, lo, hi, process_group):
    mk = importlib.import_module("make_golden")
    W = importlib.import_module(PKG + ".weights")
    M = importlib.import_module(PKG + ".model")
    TR = importlib.import_module(PKG + ".train")
    ens = M.Ensemble("repeat", dict(mk.CNN_CONF), [2, 1], torch.device("cuda"), precision="f32")
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(7, W.ensemble_shapes((2, 1), False)).items()})
    ens.cuda()
    step = TR.TrainStep(ens, lr=1e-3, criterion=criterion(), process_group=process_group)
    out = {"losses": [], "cell_hits": [], "hits": []}
    for s in range(steps):
        x, _ = mk.synth_bags(100 + s, B)
        y = targets(100 + s, B)
        masks = mk.make_masks(200 + s, [2, 1], B)
        for lvl, em in enumerate(ens.mla.embedded_mappings):
            for j, d in enumerate(em.dropouts):
                d.mask = masks["mla.embedded_mappings.%d.dropouts.%d" % (lvl, j)][lo:hi]
        loss, hits = step(x[lo:hi].cuda(), y[lo:hi].cuda())
        out["losses"].append(float(loss))
        out["cell_hits"].append(int(step.last_cell_hits))
        out["hits"].append(hits.tolist())
        assert step.last_counted is None
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
