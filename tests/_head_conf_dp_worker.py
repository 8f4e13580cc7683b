"""Worker of the 2-rank test of the training step at another model_conf (tests/test_head_conf_gpu.py): each rank runs ONE step of
the fused HIP TrainStep on ITS half of the global batch of tests/head_conf_cases.py (gloo, two ranks on one GPU, as
tests/_dp_worker.py) and saves the loss, the hit counts and step.grads in OUT.rank<r>.npz, its half of the CNN features -- what
the test feeds its float64 reference -- in OUT.feats<r>.npy.

    _head_conf_dp_worker.py OUT 1,1,2"""
import importlib
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
PKG = "audio-classification-using-a-deep-cnn-combined-with-multi-level-attention_amd"


def main():
    import head_conf_cases as C
    out_path, conf = sys.argv[1], tuple(int(n) for n in sys.argv[2].split(","))
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    W = importlib.import_module(PKG + ".weights")
    M = importlib.import_module(PKG + ".model")
    TR = importlib.import_module(PKG + ".train")
    case = C._case(conf)
    K, T, H = C.dims(case["kw"])
    ens = M.Ensemble("repeat", dict(C.CNN_CONF), list(conf), torch.device("cuda"))
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in C.ensemble_state(W, case).items()})
    ens.cuda()
    step = TR.TrainStep(ens, lr=C.LR)
    B = C.STEP_BAGS
    lo, hi = rank * B // world, (rank + 1) * B // world
    x, y = C.step_bags(W, 0, K, T)
    C._install(ens.mla, {k: m[lo:hi] for k, m in C.step_masks(W, 0, case).items()})
    with torch.no_grad():
        feats = ens.cnn(ens.input(x[lo:hi].cuda())).reshape(hi - lo, T, 128).cpu().numpy()
    loss, hits = step(x[lo:hi].cuda(), y[lo:hi].cuda())
    np.save(out_path + ".feats%d.npy" % rank, feats)
    np.savez(out_path + ".rank%d.npz" % rank, loss=np.array(float(loss)), hits=hits.cpu().numpy(),
             **{k: g.detach().cpu().numpy() for k, g in step.grads.items()})
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
