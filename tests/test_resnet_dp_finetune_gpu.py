"""Data-parallel finetuning of the ResNet-50 trunk (TrainStep(..., trunk_data_parallel=True)): the SyncBN backward split around
an all-reduce (mla_rn_bn_bwd_sums -> all-reduce -> mla_rn_bn_bwd_apply) at the kernel, ops and step level. Two gloo ranks share
the test GPU (tests/_resnet_dp_finetune_worker.py, launched once for the module); the RCCL transport runs on a one-rank group
with the collectives forced on, in a fresh child process. More than one rank over RCCL is not covered here."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _resnet_dp_finetune_worker as FW
from conftest import ROOT
from test_resnet_dp_gpu import ZERO_GRAD, free_port
from test_resnet_finetune_golden_gpu import check, initial_samples
from test_resnet_finetune_gpu import ensemble, nchw, nhwc, rel_max, tol      # tol: the single-call BatchNorm backward's bounds

pytestmark = pytest.mark.gpu

DW, TR, ops, RN = FW.DW, FW.TR, FW.ops, FW.RN


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    """Runs every two-rank scenario of the worker once; returns load(name) -> (rank 0 npz, rank 1 npz)."""
    out = str(tmp_path_factory.mktemp("resnet_dp_finetune") / "rn")
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("MLA_DIST_ALWAYS", None)
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_resnet_dp_finetune_worker.py"), "gloo", out],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    try:
        codes = [p.wait(timeout=900) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0, 0], codes
    return lambda name: tuple(np.load("%s.%s.rank%d.npz" % (out, name, r)) for r in range(2))


# ---- 1. kernel level, one process: stage 1 + stage 2 give the bits of the fused call ----------------------------------------------

class OneRank:
    """A SyncBN group of one whose all-reduce leaves the sums as they are: rn_bn_bwd_sync then runs both stages."""
    bn_active = True

    def __init__(self):
        self.tags = []

    def all_reduce_sum(self, t, tag="other"):
        self.tags.append((tag, t.numel(), t.dtype))
        return t


# (n, H, C): the smallest real layer shapes (layer4, layer3, layer1); 98 / 588 / 3136 rows, none a multiple of the 32-row step of a
# slice, one and two slices of 2048 rows, 98 rows: fewer than a block's 32 row lanes x 4
SPLIT_SHAPES = [(2, 7, 2048), (3, 14, 256), (1, 56, 64)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("n,H,C", SPLIT_SHAPES)
def test_split_equals_fused_bitwise(dtype, masked, n, H, C):
    g = torch.Generator().manual_seed(17 + C)
    x = (torch.randn(n, H, H, C, generator=g) * 2 + 0.5).to(dtype).cuda()
    dy = torch.randn(n, H, H, C, generator=g).to(dtype).cuda()
    bn = RN.BatchNorm2d(C).cuda()
    bn.weight.data.copy_(torch.rand(C, generator=g) + 0.5); bn.bias.data.copy_(torch.randn(C, generator=g) * 0.2)
    scale, shift, mean, var = ops.rn_bn_stats(x, bn, running=False, want_stats=True)
    y = ops.rn_bn_apply(x, scale, shift, relu=True, out=torch.empty_like(x)) if masked else None
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dx, dres = ops.rn_bn_bwd(x, dy, mean, var, bn, y=y, want_dres=True, dgamma=dg, dbeta=db)
    one = OneRank()
    dg2, db2 = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
    dx2, dres2 = ops.rn_bn_bwd_sync(x, dy, mean, var, bn, one, y=y, want_dres=True, dgamma=dg2, dbeta=db2)
    assert one.tags == [("syncbn_rn_bwd", 2 * C + 1, torch.float64)]
    assert torch.isfinite(dx.float()).all()
    for name, a, b in (("dx", dx, dx2), ("dres", dres, dres2), ("dgamma", dg, dg2), ("dbeta", db, db2)):
        assert torch.equal(a, b), name
    # no dres, no affine gradients: the same dx; without an active SyncBN group rn_bn_bwd_sync is rn_bn_bwd
    dx3, none = ops.rn_bn_bwd_sync(x, dy, mean, var, bn, OneRank(), y=y)
    assert none is None and torch.equal(dx3, dx)
    dx4, _ = ops.rn_bn_bwd_sync(x, dy, mean, var, bn, ops._local(), y=y)
    assert torch.equal(dx4, dx)


class NoRows(OneRank):
    """An all-reduce whose result carries a zero row count: what no stage 1 ever sends."""

    def all_reduce_sum(self, t, tag="other"):
        t[-1] = 0.0
        return t


def test_zero_count_poisons_dx():
    """The count of stage 2 lives in device memory, out of reach of a host-side MLA_E_ARG: a count that is not > 0 gives an
    all-NaN dx (visible at once) instead of inf / garbage coefficients; dgamma / dbeta (stage 1, local sums) are untouched."""
    C = 64
    g = torch.Generator().manual_seed(5)
    x, dy = torch.randn(2, 7, 7, C, generator=g).cuda(), torch.randn(2, 7, 7, C, generator=g).cuda()
    bn = RN.BatchNorm2d(C).cuda()
    _, _, mean, var = ops.rn_bn_stats(x, bn, running=False, want_stats=True)
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dx, _ = ops.rn_bn_bwd_sync(x, dy, mean, var, bn, NoRows(), dgamma=dg, dbeta=db)
    assert torch.isnan(dx).all() and torch.isfinite(dg).all() and torch.isfinite(db).all()


# ---- 2. unequal shards, ops level, two ranks ---------------------------------------------------------------------------------------

def test_unequal_shards_against_float64_autograd(ranks):
    """3 + 1 images of one (4, 28, 28, 128) tensor: dx / dres concatenated and dgamma / dbeta ADDED over the ranks against float64
    autograd of train-mode BatchNorm + ReLU on all 4 images, with the bounds of the single-call BatchNorm backward
    (tests/test_resnet_finetune_gpu.py: tol(float32) = 1e-4, max error relative to the largest reference element). A count of
    rows x world would be 1.5 x / 0.5 x off; dgamma written from the all-reduced sums would come out twice as large."""
    r0, r1 = ranks("unequal")
    x, dy, bn = FW.unequal_case()
    y = torch.from_numpy(np.concatenate([r0["y"], r1["y"]]))
    xr = nchw(x.double()).clone().requires_grad_(True)
    gr, br = bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True)
    out = F.batch_norm(xr, None, None, gr, br, training=True, eps=bn.eps)
    mask = (nchw(y.double()) > 0).double()                          # the kernel's mask is the kept output's sign
    assert rel_max(y, nhwc(F.relu(out.detach()))) <= tol(torch.float32)
    out.backward(nchw(dy.double()) * mask)
    got = {k: torch.from_numpy(np.concatenate([r0[k], r1[k]])) for k in ("dx", "dres")}
    got.update({k: torch.from_numpy(r0[k] + r1[k]) for k in ("dgamma", "dbeta")})
    ref = {"dx": nhwc(xr.grad), "dres": dy.double() * nhwc(mask), "dgamma": gr.grad, "dbeta": br.grad}
    for k in ("dx", "dres", "dgamma", "dbeta"):
        e = rel_max(got[k], ref[k])
        print("unequal shards 3 + 1: %s max rel %.3g" % (k, e))
        assert e <= tol(torch.float32), (k, e)
    assert r0["dx"].shape[0] == 3 and r1["dx"].shape[0] == 1
    assert not np.array_equal(r0["dgamma"], r1["dgamma"])           # each rank's own part


# ---- 3. two ranks against the reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["a", "b"])
def test_two_ranks_against_reference(ranks, golden, tag):
    """The three steps of resnet_finetune.npz a / b (the reference's single process on 2 bags, float64) as 1 + 1 bags on two
    ranks, through check() of tests/test_resnet_finetune_golden_gpu.py with its tolerances. Run b trains conv1 (and the fc) only,
    but the backward walks down to the stem through every block: 53 backward messages per step in both runs."""
    g = golden("resnet_finetune")
    r0, r1 = ranks("golden_" + tag)
    assert r0.files == r1.files
    for k in r0.files:
        if k != "out":                                             # each rank's own row of the scores
            np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)  # replicas stay bit-identical: gradients, state, buffers
    assert int(r0["syncbn_rn"]) == 3 * 53 and int(r0["syncbn_rn_bwd"]) == 3 * 53 and int(r0["grad_flat"]) == 3
    ens = FW.build_ft(FW.RUNS[tag])
    init = initial_samples(g, tag, ens)
    ens.load_state_dict({k[6:]: torch.as_tensor(r0[k]) for k in r0.files if k.startswith("state/")}, strict=True)
    grads1 = {k[5:]: torch.as_tensor(r0[k]) for k in r0.files if k.startswith("grad/")}
    scores1 = np.concatenate([r0["out"], r1["out"]])
    assert scores1.shape == (2, 10)
    check(g, tag, ens, list(r0["losses"]), scores1, grads1, init)


# ---- 4. two ranks against one process, bf16 ---------------------------------------------------------------------------------------

# Step-1 gradients of 4 bags as 2 + 2 against the single process on all 4, relative L2 per tensor (ZERO_GRAD tensors skipped).
# The split changes only the order of f32 / double sums (the two halves of a BatchNorm sum, the two halves of a weight gradient),
# so the gap must be far below the distance between the bf16 and the f32 gradients of the same step. Measured on an MI355X
# (DESIGN.md section 4): 1.44e-6 at cnn.cnn_model.4.0.conv1.weight (the loss: equal) against 0.585 between the bf16 and the f32
# gradients of the single process (worst tensor cnn.cnn_model.4.1.bn1.weight; bf16 rounding flips ReLU masks in the lower
# layers). The bound is 10 x the measured gap.
MEASURED_SPLIT_GAP = 1.44e-6


def per_tensor(ens, flat_a, flat_b):
    """Worst relative L2 over the trained tensors of two flat gradient buffers (TrainStep's seating order, 4-float aligned)."""
    off, worst, n_cmp = 0, (0.0, ""), 0
    for n, p in ens.named_parameters():
        if not p.requires_grad or ".fcf." in n:
            continue
        k = p.numel()
        if not n.endswith(ZERO_GRAD):
            a, b = flat_a[off:off + k].astype(np.float64), flat_b[off:off + k].astype(np.float64)
            worst = max(worst, (float(np.linalg.norm(a - b) / np.linalg.norm(b)), n))
            n_cmp += 1
        off += (k + 3) // 4 * 4
    assert off == flat_a.size == flat_b.size and n_cmp >= 160
    return worst


def test_two_ranks_equal_one_process_bf16(ranks):
    r0, r1 = ranks("vs1_bf16")
    np.testing.assert_array_equal(r0["flat_g"], r1["flat_g"])
    flat = {}
    for prec in ("bf16", "f32"):
        ens = FW.build_ft(FW.RUNS["a"], prec)
        step = TR.TrainStep(ens, lr=FW.LR, graph=False)
        DW.inject(ens, 300, 4)
        loss = float(step(DW.images(40, 4), DW.labels(4))[0])
        flat[prec] = step.flat_g.cpu().numpy()
        if prec == "bf16":
            e_loss = abs(float(r0["loss"]) - loss) / abs(loss)
    gap, ref_gap = per_tensor(ens, r0["flat_g"], flat["bf16"]), per_tensor(ens, flat["bf16"], flat["f32"])
    print("2 + 2 bf16 against one process: loss rel %.3g; gradients worst rel L2 %.3g at %s; bf16 against f32 (one process) %.3g at %s"
          % ((e_loss,) + gap + ref_gap))
    assert e_loss <= 1e-5
    assert gap[0] <= 10 * MEASURED_SPLIT_GAP, gap
    assert gap[0] <= 0.1 * ref_gap[0], (gap, ref_gap)                 # far below what bf16 itself costs


# ---- 5. sync_bn=False ---------------------------------------------------------------------------------------------------------------

def test_per_shard_batchnorm_gradients(ranks):
    """sync_bn=False, 2 + 2 bags, f32: no syncbn* message, and the flat gradient each rank hands to the exchange is that of a
    single process on its 2 bags with the loss scaled by 1 / 4 instead of 1 / 2 -- every operation behind the loss scale is linear
    and a factor 1/2 is exact in binary floating point, so the two are equal bit for bit."""
    both = ranks("pershard")
    for rank, r in enumerate(both):
        tags = list(r["tags"])
        assert not any(t.startswith("syncbn") for t in tags) and tags.count("grad:flat") == 1
        ens = FW.build_ft(FW.RUNS["a"])
        step = TR.TrainStep(ens, lr=FW.LR, graph=False)
        DW.inject(ens, 400, 4, 2 * rank, 2 * rank + 2)
        step(DW.images(60, 4)[2 * rank:2 * rank + 2], DW.labels(4)[2 * rank:2 * rank + 2])
        alone = step.flat_g.cpu().numpy()
        assert np.abs(alone).max() > 0
        np.testing.assert_array_equal(r["flat_g_local"], 0.5 * alone)
    np.testing.assert_array_equal(both[0]["flat_g_summed"], both[1]["flat_g_summed"])
    assert not np.array_equal(both[0]["flat_g_local"], both[1]["flat_g_local"])


# ---- 6. one-rank RCCL, collectives forced on ----------------------------------------------------------------------------------------

def test_one_rank_forced_collectives_bit_identical():
    """A one-rank RCCL group with the collectives forced on (53 forward + 53 backward SyncBN messages and the flat gradient
    through mla_allreduce_flat) against TrainStep without a group: three bf16 finetune steps, losses, flat parameters and every
    trunk running statistic torch.equal."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MLA_DIST_COLLECTIVE", "MLA_DIST_ALWAYS"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_resnet_dp_finetune_worker.py"), "nccl"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = p.stdout.decode()
    print(out[-2000:])
    assert p.returncode == 0 and "resnet finetune nccl worker ok" in out, out[-3000:]


# ---- 7. opt-in ------------------------------------------------------------------------------------------------------------------------

def test_opt_in_under_a_process_group(tmp_path):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + os.path.join(str(tmp_path), "pg"), rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match="SyncBN backward"):
            TR.TrainStep(ensemble(cnn_trainable=True))
        with pytest.raises(NotImplementedError, match="SyncBN backward"):
            TR.TrainStep(ensemble(cnn_trainable=True), trunk_data_parallel=False)
        ens = ensemble(cnn_trainable=True)
        before = ens.cnn.cnn_model[0].weight.detach().clone()
        step = TR.TrainStep(ens, lr=1e-4, trunk_data_parallel=True)
        assert step.rn_trunk and "rn_trunk" in step.buckets
        loss, _ = step(DW.images(10, 2), DW.labels(2))            # 2 bags: the head's BatchNorm1d(K) over the bags needs more than one
        assert np.isfinite(float(loss)) and not torch.equal(ens.cnn.cnn_model[0].weight.detach(), before)
    finally:
        dist.destroy_process_group()
