"""Worker of the data-parallel ResNet tests (tests/test_resnet_dp_gpu.py): cnn_type="resnet" with the frozen trunk in train mode,
its 53 BatchNorm2d statistics summed over the ranks (SyncBN) or kept per shard.

    _resnet_dp_worker.py gloo OUT    two ranks (RANK / WORLD_SIZE from the environment) sharing the test GPU over gloo; every
                                     scenario below writes OUT.<scenario>.rank<r>.npz
    _resnet_dp_worker.py nccl        one rank on backend "nccl" with the collectives forced on (ops.Dist(always=True)): the
                                     steps must equal the steps without a group, bit for bit; prints "resnet nccl worker ok"

The helpers (build, images, labels, inject) are shared with the test, which runs the single-process counterparts."""
import importlib
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "audio-classification-using-a-deep-cnn-combined-with-multi-level-attention_amd"

M = importlib.import_module(PKG + ".model")
W = importlib.import_module(PKG + ".weights")
TR = importlib.import_module(PKG + ".train")
ops = importlib.import_module(PKG + ".ops")
RN = importlib.import_module(PKG + ".resnet")

SEED = 21                 # the weights of tests/golden/resnet.npz
FRAME = 10 * 600          # dropout-mask elements per bag (T rows of H)


def conf(jb):
    return dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=jb, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)


def build(jb, precision="f32"):
    ens = M.Ensemble("repeat", conf(jb), [2, 1], torch.device("cuda"), precision=precision)
    sd = W.make_state_dict(SEED, W.ensemble_shapes((2, 1), jb, cnn_type="resnet", num_classes=10))
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    return ens.cuda()


def images(seed, bags, T=10):
    x = W.uniform(seed, W.stream_id("rn_images"), bags * T * 224 * 224, lo=0.0, hi=1.0)
    return torch.from_numpy(x.reshape(bags, T, 1, 224, 224)).cuda()


def labels(bags, seed=0):
    return torch.tensor([(3 * i + seed) % 10 for i in range(bags)], dtype=torch.long).cuda()


def inject(ens, seed, bags, lo=0, hi=None):
    """The dropout masks of a `bags`-bag single-process step, bags [lo, hi) of them (a rank's shard)."""
    hi = bags if hi is None else hi
    for lvl, em in enumerate(ens.mla.embedded_mappings):
        for j, d in enumerate(em.dropouts):
            key = "mla.embedded_mappings.%d.dropouts.%d" % (lvl, j)
            d.mask = torch.from_numpy(W.keep_mask(seed, W.stream_id(key), bags * FRAME, 0.4)[lo * FRAME:hi * FRAME])


def trunk_stats(ens):
    """The 53 x (running_mean, running_var, num_batches_tracked) of the trunk, as numpy."""
    return {k: v.cpu().numpy() for k, v in ens.cnn.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def trained_state(ens):
    """Everything a frozen-trunk step changes: head, cnn.cnn_model.fc (just_bottlenecks=False) and the trunk's buffers."""
    return {k: v.cpu().numpy() for k, v in ens.state_dict().items()
            if k.startswith(("mla.", "cnn.cnn_model.fc.")) or k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def run_steps(ens, step, steps, bags, lo, hi, img_seed, mask_seed):
    losses = []
    for s in range(steps):
        inject(ens, mask_seed + s, bags, lo, hi)
        loss, _ = step(images(img_seed + s, bags)[lo:hi], labels(bags, s)[lo:hi])
        losses.append(float(loss))
    return np.array(losses)


# ---- two gloo ranks -------------------------------------------------------------------------------------------------------------

def gloo(out):
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    assert world == 2
    pg = dist.group.WORLD

    def save(name, **arrays):
        np.savez(out + ".%s.rank%d.npz" % (name, rank), **arrays)

    # 1. the three steps of resnet.npz train/{jb,fc}: the 2-bag run split 1 + 1
    for jb in (True, False):
        ens = build(jb)
        step = TR.TrainStep(ens, lr=1e-3, process_group=pg)
        assert step.dist.active and step.dist.bn_active
        losses = run_steps(ens, step, 3, 2, rank, rank + 1, 10, 200)
        save("golden_%s" % ("jb" if jb else "fc"), losses=losses, **trained_state(ens))

    # 2. one train-mode forward of images(2, 2), one bag per rank
    ens = build(True).train()
    with torch.no_grad():
        RN.trunk_forward(ens.cnn.cnn_model, ens.input(images(2, 2)[rank:rank + 1]), "f32", True, ens.cnn._rn_cache,
                         dist=ops.Dist(pg))
    save("fwd", **trunk_stats(ens))

    # 3. 4 bags split 2 + 2, against one process (the test runs that one)
    for prec in ("f32", "bf16"):
        for jb in (True, False):
            ens = build(jb, prec)
            step = TR.TrainStep(ens, lr=1e-3, process_group=pg)
            step.dist.trace = []
            losses = run_steps(ens, step, 3, 4, 2 * rank, 2 * rank + 2, 40, 300)
            tags = [t[0] for t in step.dist.trace]
            save("vs1_%s_%s" % (prec, "jb" if jb else "fc"), losses=losses, flat_p=step.flat_p.cpu().numpy(),
                 syncbn_rn=tags.count("syncbn_rn"), **trunk_stats(ens))

    # 5. sync_bn=False, 2 + 2 bags: per-shard statistics; the same shard through a fresh single-process train-mode trunk
    for prec, jb in (("f32", True), ("bf16", False)):
        ens = build(jb, prec)
        step = TR.TrainStep(ens, lr=1e-3, process_group=pg, sync_bn=False)
        step.dist.trace = []
        assert step.dist.active and not step.dist.bn_active
        run_steps(ens, step, 1, 4, 2 * rank, 2 * rank + 2, 60, 400)
        assert not any(t[0].startswith("syncbn") for t in step.dist.trace)
        alone = build(jb, prec).train()
        with torch.no_grad():
            RN.trunk_forward(alone.cnn.cnn_model, alone.input(images(60, 4)[2 * rank:2 * rank + 2]), prec, True, alone.cnn._rn_cache)
        got, want = trunk_stats(ens), trunk_stats(alone)
        save("pershard_%s" % prec, **{"step/" + k: v for k, v in got.items()}, **{"alone/" + k: v for k, v in want.items()})

    # 6. ops level, unequal shards: 3 + 1 images of one NHWC tensor against one rn_bn_stats call on all 4
    C = 128
    x = torch.from_numpy(W.uniform(5, W.stream_id("rn_dp_unequal"), 4 * 28 * 28 * C, lo=-1.0, hi=3.0).reshape(4, 28, 28, C)).cuda()

    def holder():
        bn = RN.BatchNorm2d(C)
        bn.weight.data = torch.from_numpy(W.uniform(6, 1, C, lo=0.5, hi=1.5))
        bn.bias.data = torch.from_numpy(W.uniform(6, 2, C, lo=-0.5, hi=0.5))
        bn.running_mean.copy_(torch.from_numpy(W.uniform(6, 3, C, lo=-0.1, hi=0.1)))
        bn.running_var.copy_(torch.from_numpy(W.uniform(6, 4, C, lo=0.8, hi=1.2)))
        return bn.cuda()
    lo, hi = (0, 3) if rank == 0 else (3, 4)
    bn = holder()
    scale, shift = ops.rn_bn_stats_sync(x[lo:hi].contiguous(), bn, ops.Dist(pg))
    ref = holder()
    rscale, rshift = ops.rn_bn_stats(x, ref)
    save("unequal", scale=scale.cpu().numpy(), shift=shift.cpu().numpy(), running_mean=bn.running_mean.cpu().numpy(),
         running_var=bn.running_var.cpu().numpy(), tracked=int(bn.num_batches_tracked), ref_scale=rscale.cpu().numpy(),
         ref_shift=rshift.cpu().numpy(), ref_running_mean=ref.running_mean.cpu().numpy(), ref_running_var=ref.running_var.cpu().numpy())

    dist.barrier()
    dist.destroy_process_group()
    print("resnet gloo worker rank %d ok" % rank)


# ---- one RCCL rank, collectives forced on ---------------------------------------------------------------------------------------

def nccl():
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))

    def run(prec, jb, always):
        os.environ["MLA_DIST_ALWAYS"] = "1" if always else "0"
        ens = build(jb, prec)
        step = TR.TrainStep(ens, lr=1e-3, graph=False)
        assert step.dist.active == always and step.dist.bn_active == always
        step.dist.trace = [] if always else None
        losses = run_steps(ens, step, 3, 2, 0, 2, 10, 200)
        torch.cuda.synchronize()
        tags = [t[0] for t in step.dist.trace] if always else []
        via = step.dist.via
        step.dist.close()
        return losses, step.flat_p.clone(), {k: v.clone() for k, v in ens.cnn.state_dict().items() if "running" in k or "tracked" in k}, tags, via

    for prec, jb in (("f32", False), ("bf16", True)):
        base = run(prec, jb, False)
        coll = run(prec, jb, True)
        assert coll[4] == "abi", coll[4]
        assert coll[3].count("syncbn_rn") == 3 * 53, coll[3].count("syncbn_rn")
        assert np.array_equal(base[0], coll[0]), (prec, jb, base[0], coll[0])
        assert torch.equal(base[1], coll[1]), (prec, jb)
        assert len(base[2]) == 3 * 53 and base[2].keys() == coll[2].keys()
        for k in base[2]:
            assert torch.equal(base[2][k], coll[2][k]), (prec, jb, k)
        print("resnet nccl worker: %s %s losses %s, 53 trunk all-reduces per step, bit-identical" % (prec, "jb" if jb else "fc",
                                                                                                    coll[0].tolist()))
    dist.barrier()
    dist.destroy_process_group()
    print("resnet nccl worker ok")


if __name__ == "__main__":
    if sys.argv[1] == "gloo":
        gloo(sys.argv[2])
    else:
        nccl()
