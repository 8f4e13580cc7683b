"""Worker of the data-parallel ResNet trunk-finetuning tests (tests/test_resnet_dp_finetune_gpu.py): cnn_type="resnet" with
trunk parameters in the update set under a process group -- SyncBN in the trunk's forward (mla_rn_bn_sums -> all-reduce ->
mla_rn_bn_finish) AND backward (mla_rn_bn_bwd_sums -> all-reduce -> mla_rn_bn_bwd_apply), one flat gradient all-reduce.

    _resnet_dp_finetune_worker.py gloo OUT   two ranks (RANK / WORLD_SIZE from the environment) sharing the test GPU over gloo;
                                             every scenario below writes OUT.<scenario>.rank<r>.npz
    _resnet_dp_finetune_worker.py nccl       one rank on backend "nccl" with the collectives forced on (ops.Dist(always=True))
                                             against TrainStep before any group exists, bit for bit; prints
                                             "resnet finetune nccl worker ok"

The helpers (images, labels, inject, trunk_stats of _resnet_dp_worker; build_ft, unequal_case here) are shared with the test,
which runs the single-process counterparts."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

import _resnet_dp_worker as DW

M, W, TR, ops, RN = DW.M, DW.W, DW.TR, DW.ops, DW.RN
# the two runs of tests/golden/resnet_finetune.npz, as tests/test_resnet_finetune_golden_gpu.py builds them
RUNS = {"a": dict(conf="repeat", jb=True, cnn_trainable=True, first_cnn_layer_trainable=False),
        "b": dict(conf="single", jb=False, cnn_trainable=False, first_cnn_layer_trainable=True)}
LR = 1e-4


def build_ft(run, precision="f32"):
    cnn_conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=run["jb"],
                    cnn_trainable=run["cnn_trainable"], first_cnn_layer_trainable=run["first_cnn_layer_trainable"], in_channels=3)
    ens = M.Ensemble(run["conf"], cnn_conf, [2, 1], torch.device("cuda"), precision=precision, trunk_backward=True)
    sd = W.make_state_dict(DW.SEED, W.ensemble_shapes((2, 1), run["jb"], cnn_type="resnet", num_classes=10))
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    return ens.cuda()


def unequal_case():
    """x, dy (4, 28, 28, 128) f32 and the BatchNorm2d holder of the 3 + 1 scenario."""
    C = 128
    x = torch.from_numpy(W.uniform(5, W.stream_id("rn_dp_unequal"), 4 * 28 * 28 * C, lo=-1.0, hi=3.0).reshape(4, 28, 28, C))
    dy = torch.from_numpy(W.uniform(7, W.stream_id("rn_dp_unequal_dy"), 4 * 28 * 28 * C, lo=-1.0, hi=1.0).reshape(4, 28, 28, C))
    bn = RN.BatchNorm2d(C)
    bn.weight.data = torch.from_numpy(W.uniform(6, 1, C, lo=0.5, hi=1.5))
    bn.bias.data = torch.from_numpy(W.uniform(6, 2, C, lo=-0.5, hi=0.5))
    return x, dy, bn


def np_grads(step):
    return {"grad/" + n: t.cpu().numpy() for n, t in step.grads.items()}


def np_state(ens):
    return {"state/" + k: v.cpu().numpy() for k, v in ens.state_dict().items()}


def count(trace, tag):
    return sum(t[0] == tag for t in trace)


# ---- two gloo ranks -------------------------------------------------------------------------------------------------------------

def gloo(out):
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    assert world == 2
    pg = dist.group.WORLD

    def save(name, **arrays):
        np.savez(out + ".%s.rank%d.npz" % (name, rank), **arrays)

    # 2. ops level, unequal shards: 3 + 1 images through rn_bn_stats_sync, then rn_bn_bwd_sync with the ReLU mask
    x, dy, bn = unequal_case()
    lo, hi = (0, 3) if rank == 0 else (3, 4)
    xs, dys, bn, d = x[lo:hi].contiguous().cuda(), dy[lo:hi].contiguous().cuda(), bn.cuda(), ops.Dist(pg)
    d.trace = []
    scale, shift, mean, var = ops.rn_bn_stats_sync(xs, bn, d, running=False, want_stats=True)
    y = ops.rn_bn_apply(xs, scale, shift, relu=True, out=torch.empty_like(xs))
    dgamma, dbeta = torch.empty(128, device="cuda"), torch.empty(128, device="cuda")
    dx, dres = ops.rn_bn_bwd_sync(xs, dys, mean, var, bn, d, y=y, want_dres=True, dgamma=dgamma, dbeta=dbeta)
    assert [t[:2] for t in d.trace] == [("syncbn_rn", 8 * 257), ("syncbn_rn_bwd", 8 * 257)]
    save("unequal", y=y.cpu().numpy(), dx=dx.cpu().numpy(), dres=dres.cpu().numpy(), dgamma=dgamma.cpu().numpy(),
         dbeta=dbeta.cpu().numpy())

    # 3. the three steps of resnet_finetune.npz a / b (the reference's single process on 2 bags) as 1 + 1 bags
    for tag, run in RUNS.items():
        ens = build_ft(run)
        step = TR.TrainStep(ens, lr=LR, process_group=pg, trunk_data_parallel=True)
        assert step.dist.active and step.dist.bn_active and step.rn_trunk
        step.dist.trace = []
        losses, first = [], {}
        for s in range(3):
            DW.inject(ens, 200 + s, 2, rank, rank + 1)
            losses.append(float(step(DW.images(10 + s, 2)[rank:rank + 1], DW.labels(2, s)[rank:rank + 1])[0]))
            if s == 0:
                first = dict(np_grads(step), out=step.last_out.cpu().numpy())
        assert step._graph is None
        tr = step.dist.trace
        save("golden_" + tag, losses=np.array(losses), syncbn_rn=count(tr, "syncbn_rn"), syncbn_rn_bwd=count(tr, "syncbn_rn_bwd"),
             grad_flat=count(tr, "grad:flat"), n_collectives=len(tr), **first, **np_state(ens))
        del ens, step, first
        torch.cuda.empty_cache()

    # 4. bf16, 4 bags as 2 + 2, one step: the gradients after the exchange against one process on all 4 (the test runs that one)
    ens = build_ft(RUNS["a"], "bf16")
    step = TR.TrainStep(ens, lr=LR, process_group=pg, trunk_data_parallel=True)
    DW.inject(ens, 300, 4, 2 * rank, 2 * rank + 2)
    loss = float(step(DW.images(40, 4)[2 * rank:2 * rank + 2], DW.labels(4)[2 * rank:2 * rank + 2])[0])
    save("vs1_bf16", loss=loss, flat_g=step.flat_g.cpu().numpy())
    del ens, step
    torch.cuda.empty_cache()

    # 5. sync_bn=False, 2 + 2 bags, f32: per-shard BatchNorm forward and the fused backward, no statistics message; the flat
    # gradient as it ENTERS the exchange (observed at the gradient all-reduce) is this shard's own backward with the loss
    # scaled by 1 / 4
    ens = build_ft(RUNS["a"])
    step = TR.TrainStep(ens, lr=LR, process_group=pg, sync_bn=False, trunk_data_parallel=True)
    assert step.dist.active and not step.dist.bn_active
    step.dist.trace, seen = [], {}
    reduce = step.dist.all_reduce_sum

    def observed(t, tag="other"):
        if tag == "grad:flat":
            seen["flat_g"] = t.cpu().numpy().copy()
        return reduce(t, tag)
    step.dist.all_reduce_sum = observed
    DW.inject(ens, 400, 4, 2 * rank, 2 * rank + 2)
    step(DW.images(60, 4)[2 * rank:2 * rank + 2], DW.labels(4)[2 * rank:2 * rank + 2])
    tags = [t[0] for t in step.dist.trace]
    assert not any(t.startswith("syncbn") for t in tags), tags
    assert tags.count("grad:flat") == 1 and "flat_g" in seen
    save("pershard", flat_g_local=seen["flat_g"], flat_g_summed=step.flat_g.cpu().numpy(), tags=np.array(tags))

    dist.barrier()
    dist.destroy_process_group()
    print("resnet finetune gloo worker rank %d ok" % rank)


# ---- one RCCL rank, collectives forced on ---------------------------------------------------------------------------------------

def nccl():
    torch.cuda.set_device(0)

    def run(always):
        os.environ["MLA_DIST_ALWAYS"] = "1" if always else "0"          # ops.Dist(always=True) inside TrainStep
        ens = build_ft(RUNS["a"], "bf16")
        step = TR.TrainStep(ens, lr=LR, graph=False, trunk_data_parallel=always)
        step.dist.trace = [] if always else None
        assert step.dist.active == always and step.dist.bn_active == always
        losses = DW.run_steps(ens, step, 3, 2, 0, 2, 10, 200)
        torch.cuda.synchronize()
        tags = [t[0] for t in step.dist.trace] if always else []
        via = step.dist.via
        step.dist.close()
        return losses, step.flat_p.clone(), {k: v.clone() for k, v in ens.cnn.state_dict().items() if "running" in k or "tracked" in k}, tags, via

    assert not dist.is_initialized()
    base = run(False)                                  # TrainStep without a group: before any process group exists
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    coll = run(True)
    assert coll[4] == "abi", coll[4]
    assert coll[3].count("syncbn_rn") == 3 * 53 and coll[3].count("syncbn_rn_bwd") == 3 * 53, coll[3]
    assert coll[3].count("grad:flat") == 3
    assert np.array_equal(base[0], coll[0]), (base[0], coll[0])
    assert torch.equal(base[1], coll[1])
    assert len(base[2]) == 3 * 53 and base[2].keys() == coll[2].keys()
    for k in base[2]:
        assert torch.equal(base[2][k], coll[2][k]), k
    print("resnet finetune nccl worker: bf16 losses %s, 53 + 53 trunk all-reduces per step, bit-identical" % coll[0].tolist())
    dist.barrier()
    dist.destroy_process_group()
    print("resnet finetune nccl worker ok")


if __name__ == "__main__":
    if sys.argv[1] == "gloo":
        gloo(sys.argv[2])
    else:
        nccl()
