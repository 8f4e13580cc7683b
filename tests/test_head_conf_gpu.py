"""GPU tests of the trained head at model_conf other than [2, 1]: depths 1 to 4, up to 3 layers per level, input width 10 (the small
Linear at level 0), the wide pooling / BatchNorm path at an odd class count, 50 classes. What depends on the depth: the
two-consumer accumulation of mla_backward (a middle level, a single level), the column slices of the concatenation (pitch L K,
offsets lvl K), want_dx at the bottom of the walk, a third tape record and dropout stream per level, and the flat-buffer layout of
TrainStep. Cases, float64 reference, tolerances: tests/head_conf_cases.py; that a HIP result outside a tolerance is a defect and
that the tolerances see the defects these cases are for: tests/test_head_conf_cases_cpu.py."""

import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import head_conf_cases as C
from conftest import PKG, ROOT
from test_train_gpu import free_port

pytestmark = pytest.mark.gpu

IDS = [C.case_id(c) for c in C.HEAD_CASES]
MODE_IDS = ["eval", "train"]


@pytest.fixture(scope="module")
def M():
    return importlib.import_module(PKG + ".model")


@pytest.fixture(scope="module")
def TR():
    return importlib.import_module(PKG + ".train")


def build_head(M, W, case, train):
    mla = M.MultiLevelAttention(list(case["conf"]), case["width"], **case["kw"])
    mla.load_state_dict({k[len("mla."):]: torch.as_tensor(v) for k, v in C.head_state(W, case).items()})
    mla.cuda().train(train)
    return mla


def run_head(M, W, case, train, input_grad=True):
    """One forward and backward of sum(out * wgt) through MultiLevelAttention.__call__ (HeadFn) -> (the result in run_oracle's
    layout, the module)."""
    K, T, H = C.dims(case["kw"])
    x, wgt, masks = C.head_inputs(W, case, train)
    mla = build_head(M, W, case, train)
    if train:
        C._install(mla, masks)
    before = {k: v.clone() for k, v in mla.state_dict().items() if k.endswith(C.STATS)}
    xg = x.cuda().requires_grad_(input_grad)
    out = mla(xg)
    assert tuple(out.shape) == (C.BAGS, K) and out.requires_grad
    after = {k: v.clone() for k, v in mla.state_dict().items() if k.endswith(C.STATS)}
    for k, v in after.items():
        if train:
            assert not k.endswith("num_batches_tracked") or int(v) == 1, k
        else:
            assert torch.equal(v, before[k]), k                    # eval mode leaves every buffer alone
    (out * wgt.cuda()).sum().backward()
    res = {"out": out.detach(), "dx": xg.grad, "grads": {n: p.grad for n, p in mla.named_parameters()},
           "running": {k: v for k, v in after.items() if train and not k.endswith("num_batches_tracked")}}
    return res, mla


# ------------------------------------------------------------------------------------- 3.1 head against float64 ----

@pytest.mark.parametrize("train", [False, True], ids=MODE_IDS)
@pytest.mark.parametrize("case", C.HEAD_CASES, ids=IDS)
def test_head_matches_the_oracle_in_float64(M, W, case, train):
    """Every head case in eval mode (running statistics away from their initial values) and train mode (batch statistics, injected
    masks), 6 bags, through HeadFn with an input that requires grad: the output, the running statistics after the train-mode
    forward with num_batches_tracked == 1, the input gradient and every parameter gradient against float64 autograd through
    oracle.model.mla_forward on the same state_dict. fcf receives no gradient."""
    ref = C.reference(W, case, train)
    got, _ = run_head(M, W, case, train)
    assert set(got["grads"]) == set(ref["grads"]) and set(got["running"]) == set(ref["running"])
    for n, g in got["grads"].items():
        assert (g is None) == (".fcf." in n) and (ref["grads"][n] is None) == (".fcf." in n), n
    assert got["dx"] is not None and tuple(got["dx"].shape) == tuple(ref["dx"].shape)
    C.report("head %s train=%s" % (C.case_id(case), train), C.shares(got, ref))


# ------------------------------------------------------------------------------ 3.2 without an input gradient ----

@pytest.mark.parametrize("train", [False, True], ids=MODE_IDS)
@pytest.mark.parametrize("conf", [(1,), (1, 1, 2)], ids=["conf1", "conf112"])
def test_parameter_gradients_do_not_depend_on_the_input_gradient(M, W, conf, train):
    """x.requires_grad == False: the want_dx=False branch of the BatchNorm backward at level 0 (with one level, the only norm0 there
    is). Everything but dx against float64, and every parameter gradient bit for bit as in the run with an input gradient."""
    case = C._case(conf)
    ref = C.reference(W, case, train)
    got, _ = run_head(M, W, case, train, input_grad=False)
    assert got["dx"] is None
    C.report("head without dx %s train=%s" % (C.case_id(case), train), C.shares(got, ref))
    with_dx, _ = run_head(M, W, case, train, input_grad=True)
    assert torch.equal(got["out"], with_dx["out"])
    for n, g in with_dx["grads"].items():
        if ".fcf." in n:
            assert g is None and got["grads"][n] is None, n
        else:
            assert torch.equal(got["grads"][n], g), n


# --------------------------------------------------------------------------------------- 3.3 bag independence ----

@pytest.mark.parametrize("conf", [(1, 1, 2), (3,)], ids=["conf112", "conf3"])
def test_eval_mode_bag_scores_do_not_depend_on_the_batch(M, W, conf):
    """Eval mode: a bag scored alone equals its row of the 6-bag batch bit for bit, without and behind autograd."""
    case = C._case(conf)
    x, _, _ = C.head_inputs(W, case, False)
    mla = build_head(M, W, case, False)
    with torch.no_grad():
        batch = mla(x.cuda())
        for b in range(C.BAGS):
            assert torch.equal(mla(x[b:b + 1].cuda())[0], batch[b]), b
    assert torch.equal(mla(x.cuda()).detach(), batch)              # HeadFn's forward
    for b in (0, C.BAGS - 1):
        assert torch.equal(mla(x[b:b + 1].cuda()).detach()[0], batch[b]), b


# ---------------------------------------------------------------------------------------------- 3.4 TrainStep ----

def build_ensemble(M, W, case):
    torch.manual_seed(77)                                        # Dropout reads the seed at construction
    sd = C.ensemble_state(W, case)
    ens = M.Ensemble("repeat", dict(C.CNN_CONF), list(case["conf"]), torch.device("cuda"), **case["kw"])
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return ens.cuda(), sd


def head_state_of(ens):
    return {k: v.detach().clone().cpu() for k, v in ens.state_dict().items() if k.startswith("mla.")}


@pytest.mark.parametrize("case", C.STEP_CASES, ids=[C.case_id(c) for c in C.STEP_CASES])
def test_train_step_matches_float64_restarted_at_every_step(M, TR, W, case):
    """Frozen-VGGish Ensemble, 4 bags, 3 eager steps with injected masks, host and device labels alternating. The reference is
    restarted from the model at every step (three Adam steps of an independent float64 run turn rounding noise on near-zero
    gradients into differences of lr): before a step the model's state_dict goes to float64, mla_forward(train=True) +
    F.cross_entropy on the model's own CNN features give the loss, the hit count, the gradients and the running statistics the
    step must reproduce: loss rel 1e-4, hits exactly (the reference's top-2 margin is above 1e-4), step.grads and the running
    statistics to the head tolerances (mla.fc.bias, a mathematically zero gradient that float32 autograd alone misses over 4 bags,
    to 4 x the float32 oracle's distance: STEP_LIMITS), num_batches_tracked == step. The update on its own: the step's float32 gradients fed to a
    float64 torch.optim.Adam whose state is carried over the three steps, p_after - p_before within adam_update_bound (the Adam
    kernel's bound of tests/test_train_kernels_gpu.py on the update plus the one float32 rounding of the stored parameter; the
    CPU test shows that float32 arithmetic alone misses the former); fcf keeps its bits."""
    conf = case["conf"]
    K, T, H = C.dims(case["kw"])
    tag = "trainstep " + C.case_id(case)
    ens, sd = build_ensemble(M, W, case)
    step = TR.TrainStep(ens, lr=C.LR, graph=False)
    keys = [k for k in sd if k.startswith("mla.") and not k.endswith(C.STATS) and ".fcf." not in k]
    assert list(step.grads) == keys and step.n_params == sum(sd[k].size for k in keys)
    p64 = {k: torch.zeros(sd[k].shape, dtype=torch.float64, requires_grad=True) for k in keys}
    opt = torch.optim.Adam([p64[k] for k in keys], lr=C.LR)
    for s in range(C.STEPS):
        x, y = C.step_bags(W, s, K, T)
        masks = C.step_masks(W, s, case)
        C._install(ens.mla, masks)
        with torch.no_grad():
            feats = ens.cnn(ens.input(x.cuda())).reshape(C.STEP_BAGS, T, 128).double().cpu()
        before = head_state_of(ens)
        ref = C.step_reference(before, feats, y, conf, masks)
        print("MEASURE %s step %d: reference top-2 margin %.3g" % (tag, s, ref["margin"]))
        assert ref["margin"] > C.MARGIN
        loss, hits = step(x.cuda(), y if s % 2 else y.cuda())       # host and device labels alternate
        after = head_state_of(ens)
        grads = {k: step.grads[k].detach().clone().cpu() for k in keys}
        print("MEASURE %s step %d loss: %.3g of %.3g" % (tag, s, abs(float(loss) - ref["loss"]) / ref["loss"], C.LOSS_REL))
        assert float(loss) == pytest.approx(ref["loss"], rel=C.LOSS_REL), s
        assert hits.tolist() == [ref["hits"], 0], (s, hits.tolist(), ref["hits"])
        assert all(ref["grads"][k] is None for k in ref["grads"] if ".fcf." in k)
        sh = C.grad_shares(grads, {k: ref["grads"][k] for k in keys})
        for k, want in ref["running"].items():
            sh[k] = C.share(after[k], want, C.OUT_RTOL, C.OUT_ATOL)
            assert int(after[k.rsplit(".", 1)[0] + ".num_batches_tracked"]) == s + 1, k
        print("MEASURE %s step %d mla.fc.bias: share of the tolerance %.3g of %.3g" % (tag, s, sh["mla.fc.bias"], C.STEP_LIMITS["mla.fc.bias"]))
        C.report("%s step %d" % (tag, s), sh, limits=C.STEP_LIMITS)
        worst = (0.0, None)
        with torch.no_grad():
            for k in keys:
                p64[k].copy_(before[k].double())
                p64[k].grad = grads[k].double()
        opt.step()
        for k in keys:
            got, want = after[k].double() - before[k].double(), p64[k].detach() - before[k].double()
            worst = max(worst, (float(((got - want).abs() / C.adam_update_bound(want, before[k], after[k])).max()), k))
        print("MEASURE %s step %d Adam update: worst share of the bound %.3g (%s)" % ((tag, s) + worst))
        assert worst[0] <= 1.0, worst
        for k in after:
            if ".fcf." in k:
                assert torch.equal(after[k], torch.as_tensor(sd[k])), k
    assert step.t == C.STEPS and step._graph is None


# ------------------------------------------------------------------------------------------ 3.5 graph = eager ----

@pytest.mark.parametrize("case", C.GRAPH_CASES, ids=[C.case_id(c) for c in C.GRAPH_CASES])
def test_train_step_graph_equals_eager(M, TR, W, case):
    """The step as one HIP graph against the same steps run eagerly, masks drawn on the device, the dropout ordinals aligned between
    the two models (as test_train_step_graph_equals_eager_at_50_classes): losses, hit counts, flat_p / flat_m / flat_v and every
    entry of state_dict() bit for bit; the graphed run records exactly one graph. The graph's dropout bases are keyed by module,
    one per layer: three streams at (3,), four at (1, 1, 2)."""
    K, T, H = C.dims(case["kw"])
    runs, ords = [], None
    for graph in (False, True):
        ens, _ = build_ensemble(M, W, case)
        drops = [m for m in ens.mla.modules() if type(m).__name__ == "Dropout"]
        assert len(drops) == sum(case["conf"])
        if ords is None:
            ords = [d.ordinal for d in drops]
        for d, o in zip(drops, ords):                              # the mask stream is keyed by the module's ordinal: same for both
            d.ordinal = o
        step = TR.TrainStep(ens, lr=C.LR, graph=graph)
        out = []
        for s in range(C.STEPS):
            x, y = C.step_bags(W, s, K, T)
            loss, hits = step(x.cuda(), y.cuda() if s % 2 else y)
            out.append((float(loss), hits.tolist()))
        assert (step._graph is not None) == graph and step.t == C.STEPS
        assert step.captures == (1 if graph else 0)
        runs.append((out, step, ens))
    (ref, step_e, ens_e), (got, step_g, ens_g) = runs
    assert got == ref, (got, ref)
    assert torch.equal(step_g.flat_p, step_e.flat_p) and torch.equal(step_g.flat_m, step_e.flat_m) and torch.equal(step_g.flat_v, step_e.flat_v)
    sd_g, sd_e = ens_g.state_dict(), ens_e.state_dict()
    assert list(sd_g) == list(sd_e)
    for k in sd_g:
        assert torch.equal(sd_g[k], sd_e[k]), k


# ---------------------------------------------------------------------------------------------- 3.6 two ranks ----

def test_two_ranks_match_float64_on_the_global_batch(W, tmp_path):
    """ONE step of (1, 1, 2) on two ranks (gloo, both on the one GPU), each on its half of the 4-bag batch: rank 0's loss, hit count
    and gradients against the float64 reference of the GLOBAL batch (SyncBN sums, 1 / B_global loss scaling, one gradient
    all-reduce), fed the ranks' own CNN features; rank 1's results equal rank 0's bit for bit."""
    case = C.DP_CASE
    K, T, H = C.dims(case["kw"])
    out = str(tmp_path / "dp")
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_head_conf_dp_worker.py"), out, ",".join(map(str, case["conf"]))],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    try:
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    r0, r1 = np.load(out + ".rank0.npz"), np.load(out + ".rank1.npz")
    feats = torch.from_numpy(np.concatenate([np.load(out + ".feats%d.npy" % r) for r in range(2)]))
    assert tuple(feats.shape) == (C.STEP_BAGS, T, 128)
    sd = C.ensemble_state(W, case)
    _, y = C.step_bags(W, 0, K, T)
    ref = C.step_reference({k: torch.as_tensor(v) for k, v in sd.items() if k.startswith("mla.")}, feats, y, case["conf"],
                           C.step_masks(W, 0, case))
    assert ref["margin"] > C.MARGIN
    keys = [k for k in sd if k.startswith("mla.") and not k.endswith(C.STATS) and ".fcf." not in k]
    assert sorted(r0.files) == sorted(keys + ["loss", "hits"])
    print("MEASURE two ranks loss: %.3g of %.3g" % (abs(float(r0["loss"]) - ref["loss"]) / ref["loss"], C.LOSS_REL))
    assert float(r0["loss"]) == pytest.approx(ref["loss"], rel=C.LOSS_REL)
    assert r0["hits"].tolist() == [ref["hits"], 0]
    C.report("two ranks " + C.case_id(case), C.grad_shares({k: r0[k] for k in keys}, {k: ref["grads"][k] for k in keys}), limits=C.STEP_LIMITS)
    assert sorted(r1.files) == sorted(r0.files)
    for k in r0.files:
        np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)      # replicas stay bit-identical
