"""cnn_type="resnet" under data parallelism: the frozen trunk's 53 BatchNorm2d layers in train mode with the statistics of the
global batch (SyncBN: mla_rn_bn_sums -> all-reduce -> mla_rn_bn_finish) or of each shard (sync_bn=False). Two gloo ranks share
the test GPU (tests/_resnet_dp_worker.py, launched once for the module); the RCCL transport runs on a one-rank group with the
collectives forced on, in a fresh child process."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _resnet_dp_worker as DW
from conftest import ROOT
from test_resnet_golden_gpu import NOISY, _check_training

pytestmark = pytest.mark.gpu


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    """Runs every two-rank scenario of the worker once; returns load(name) -> (rank 0 npz, rank 1 npz)."""
    out = str(tmp_path_factory.mktemp("resnet_dp") / "rn")
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_resnet_dp_worker.py"), "gloo", out],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    try:
        codes = [p.wait(timeout=900) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0, 0], codes
    return lambda name: tuple(np.load("%s.%s.rank%d.npz" % (out, name, r)) for r in range(2))


def rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


@pytest.mark.parametrize("jb", [True, False])
def test_two_ranks_against_reference(ranks, golden, jb):
    """The three steps of resnet.npz train/{jb,fc} (the reference's single process on 2 bags) as 1 + 1 bags on two ranks."""
    g = golden("resnet")
    r0, r1 = ranks("golden_%s" % ("jb" if jb else "fc"))
    assert r0.files == r1.files
    for k in r0.files:
        np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)              # replicas stay bit-identical, buffers included
    assert sum(k.endswith("running_mean") for k in r0.files if k.startswith("cnn.")) == 53
    ens = DW.build(jb)
    ens.load_state_dict({k: torch.as_tensor(r0[k]) for k in r0.files if k != "losses"}, strict=False)
    for k, v in ens.cnn.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 3, k
    _check_training(g, "train/%s" % ("jb" if jb else "fc"), ens, list(r0["losses"]))


def test_two_rank_forward_running_statistics(ranks, golden):
    """One train-mode trunk forward of images(2, 2), one bag per rank: the reference's running statistics of both bags."""
    g = golden("resnet")
    for r in ranks("fwd"):
        worst, n = 0.0, 0
        for k in r.files:
            if k.endswith("num_batches_tracked"):
                assert int(r[k]) == int(g["trainfwd/" + k]) == 1, k
                n += 1
            else:
                worst = max(worst, rel(r[k], g["trainfwd/" + k]))
        print("two-rank forward: running statistics worst rel %.3g" % worst)
        assert n == 53 and worst <= 1e-5


# Parameters whose gradient is mathematically zero: the biases in front of a train-mode BatchNorm (NOISY) and normv.bias (the
# softmax's shift invariance, as tests/test_autograd_gpu.py states). Adam turns their rounding-noise gradients into +-lr steps
# whose sign depends on the summation order, so they are not compared.
ZERO_GRAD = NOISY + ("normv.bias",)
# Measured on an MI355X: losses 2e-7, parameters 1.2e-6 (relative L2 per tensor; bf16 included, because the
# trunk statistics of the 2 + 2 split come out bit-equal to the single process), running statistics exact.
TOL = 1e-5


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("jb", [True, False])
def test_two_ranks_equal_one_process(ranks, prec, jb):
    """4 bags as 2 + 2 on two ranks against one process on all 4: losses, trained parameters, 53 x 2 running statistics."""
    r0, r1 = ranks("vs1_%s_%s" % (prec, "jb" if jb else "fc"))
    for k in r0.files:
        np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)
    assert int(r0["syncbn_rn"]) == 3 * 53
    ens = DW.build(jb, prec)
    step = DW.TR.TrainStep(ens, lr=1e-3, graph=False)
    losses = DW.run_steps(ens, step, 3, 4, 0, 4, 40, 300)
    e_loss = rel(r0["losses"], losses)
    flat, off, e_par, n_par = step.flat_p.cpu().numpy().astype(np.float64), 0, 0.0, 0
    for n, p in ens.named_parameters():                   # the flat buffer's layout: TrainStep's seating order, 4-float aligned
        if not p.requires_grad or ".fcf." in n:
            continue
        k = p.numel()
        if not n.endswith(ZERO_GRAD):
            a, b = r0["flat_p"][off:off + k].astype(np.float64), flat[off:off + k]
            e_par = max(e_par, float(np.linalg.norm(a - b) / np.linalg.norm(b)))
            n_par += 1
        off += (k + 3) // 4 * 4
    assert off == flat.size and n_par >= 10
    stats = DW.trunk_stats(ens)
    e_stat = max(rel(r0[k], v) for k, v in stats.items() if not k.endswith("num_batches_tracked"))
    print("%s %s: losses %.3g, parameters %.3g, running statistics %.3g" % (prec, "jb" if jb else "fc", e_loss, e_par, e_stat))
    assert e_loss <= TOL and e_par <= TOL and e_stat <= TOL
    assert all(int(r0[k]) == 3 for k in stats if k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_per_shard_batchnorm(ranks, prec):
    """sync_bn=False, 2 + 2 bags: each rank's trunk running statistics are those of a single-process train-mode forward on its own
    2 bags, bit for bit (and the two ranks' differ)."""
    r0, r1 = ranks("pershard_%s" % prec)
    for r in (r0, r1):
        keys = [k[5:] for k in r.files if k.startswith("step/")]
        assert len(keys) == 3 * 53
        for k in keys:
            np.testing.assert_array_equal(r["step/" + k], r["alone/" + k], err_msg=k)
    assert any(not np.array_equal(r0["step/" + k], r1["step/" + k]) for k in keys)


def test_unequal_shards_ops_level(ranks):
    """rn_bn_stats_sync on 3 + 1 images: the statistics of one rn_bn_stats call on all 4 (the count travels in the message)."""
    for r in ranks("unequal"):
        for k in ("scale", "shift", "running_mean", "running_var"):
            e = rel(r[k], r["ref_" + k])
            assert e <= 1e-6, (k, e)
        assert int(r["tracked"]) == 1


def test_one_rank_forced_collectives_bit_identical():
    """A one-rank RCCL group with the collectives forced on (sums -> mla_allreduce_flat -> finish for each of the 53 layers) against
    TrainStep without a group: losses, flat parameters and every trunk running statistic torch.equal over 3 steps."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MLA_DIST_COLLECTIVE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_resnet_dp_worker.py"), "nccl"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    out = p.stdout.decode()
    print(out[-2000:])
    assert p.returncode == 0 and "resnet nccl worker ok" in out, out[-3000:]
