"""Multi-label training on the GPU (mla_bce; ops.bce_loss; TrainStep(criterion=nn.BCELoss); train_model(extended_criterion=True)):
the kernels against the float64 restatement of tests/bce_cases.py, saturation against torch's float32 result, bad cells, NaN,
determinism, the step against torch autograd with the same criterion, eager against graph replays, a wide head, two data-parallel
ranks and the epoch loop with its mAP report.

Kernel bounds: the yardstick is the float64 restatement on the same float32 inputs; the loss error is relative to max(|loss|, 1),
the dprobs error is the maximum error over max|reference| (bce_cases.rel). MEASURED holds (the worst value over all GPU_SHAPES x
OPTIONS, 4 x that value): the factor 4 is the margin tests/test_train_kernels_gpu.py gives every kernel."""

import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _bce_dp_worker as worker
import bce_cases as C
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

ops = importlib.import_module(PKG + ".ops")
M = importlib.import_module(PKG + ".model")
TR = importlib.import_module(PKG + ".train")

MEASURED = {"bce loss": (1.76e-7, 4 * 1.76e-7), "bce dprobs": (1.14e-7, 4 * 1.14e-7)}

NOISY = ("fc.bias", "fc.0.bias", "fc.1.bias", "fcv.bias")     # zero-gradient biases: see test_oracle_golden.py


def strided(t, left=2, right=1):
    """The same values as a column slice of a wider CUDA tensor (pitch = cols + left + right); the rest holds a value that would
    wreck any sum it entered."""
    buf = torch.full((t.shape[0], t.shape[1] + left + right), 1e30, dtype=t.dtype, device="cuda")
    view = buf[:, left:left + t.shape[1]]
    view.copy_(t)
    return view


def run_kernel(p, y, w, reduction, want_grad=True, inv_total=None):
    wd = None if w is None else torch.from_numpy(w).cuda()
    return ops.bce_loss(strided(torch.from_numpy(p)), strided(torch.from_numpy(y), left=1, right=3), wd, reduction, inv_total=inv_total,
                        want_grad=want_grad)


# ------------------------------------------------------------------ the kernels --------------------------------------------------

@pytest.mark.parametrize("rows,K", C.GPU_SHAPES)
def test_kernel_against_the_float64_restatement(rows, K):
    """One wavefront per row, four rows per workgroup, lanes striding over K: K = 1, below, at and above one stride, in a third
    stride, at 527 and at all 16 strides; fewer rows than a workgroup holds, exactly four, one more, more than the finish
    workgroup's 256 threads and more than four times that. p and the targets are column slices of wider tensors filled with 1e30.
    Options: {no weights, weights 0.25 .. 4 with one zero} x {mean, sum}. want_grad=False gives the same loss and counter bits.
    Bounds: MEASURED. Observed maxima over all cases on the MI355X: loss 1.76e-7 (1 x 63), dprobs 1.14e-7 (9 x 130); the host
    simulation (logf where the device has __logf) gives 1.05e-7 and 1.39e-7 over its shapes."""
    b_loss, b_dp = MEASURED["bce loss"][1], MEASURED["bce dprobs"][1]
    p, y = C.make_case(rows, K, 700 + rows + K)
    w = C.make_weights(K)
    worst = [0.0, 0.0]
    for weighted, reduction in C.OPTIONS:
        wk = w if weighted else None
        ref = C.restated(p, y, wk, reduction)
        loss, d, hits, cell_hits = run_kernel(p, y, wk, reduction)
        assert d.is_contiguous() and tuple(d.shape) == (rows, K)
        d = d.cpu().numpy()
        e_loss, e_dp = C.loss_err(float(loss), ref["loss"]), C.rel(d, ref["dp"])
        worst = [max(worst[0], e_loss), max(worst[1], e_dp)]
        print("%d x %d weights %s %s: loss error %.3g (bound %.3g), dprobs error %.3g (bound %.3g)"
              % (rows, K, weighted, reduction, e_loss, b_loss, e_dp, b_dp))
        assert e_loss < b_loss and e_dp < b_dp, (weighted, reduction, e_loss, e_dp)
        assert hits.tolist() + cell_hits.tolist() == ref["counts"]
        assert ops.raise_on_bad_targets(hits) == ref["counts"][0]
        loss2, d2, hits2, cell2 = run_kernel(p, y, wk, reduction, want_grad=False)
        assert d2 is None and torch.equal(loss2, loss) and torch.equal(hits2, hits) and torch.equal(cell2, cell_hits)
    print("MEASURE bce %d x %d: worst loss error %.3g, worst dprobs error %.3g" % (rows, K, worst[0], worst[1]))


def test_a_handed_in_scale_is_the_global_batch_s():
    p, y = C.make_case(5, 65, 705)
    ref = C.restated(p, y, None, "mean", inv_total=1.0 / (10 * 65))
    loss, d, _, _ = run_kernel(p, y, None, "mean", inv_total=1.0 / (10 * 65))
    assert C.loss_err(float(loss), ref["loss"]) < MEASURED["bce loss"][1] and C.rel(d.cpu().numpy(), ref["dp"]) < MEASURED["bce dprobs"][1]


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return 0.0 if a == b else abs(float(a) - float(b)) / float(np.spacing(np.abs(b)))


def torch_f32(p, y, w, reduction):
    p32 = torch.tensor(p, dtype=torch.float32).requires_grad_(True)
    loss = torch.nn.functional.binary_cross_entropy(p32, torch.tensor(y, dtype=torch.float32), weight=None if w is None else torch.tensor(w),
                                                    reduction=reduction)
    loss.backward()
    return float(loss.detach()), p32.grad.numpy()


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_saturation_equals_torch_float32(reduction):
    """As tests/test_bce_cpu.py's: the four corners alone (1 x 1, the terms 100 w and 0 are exact) and together (2 x 2), against
    torch's float32 CPU result: equal losses, gradients within one unit in the last place."""
    w1 = np.array([0.75], dtype=np.float32)
    for (pc, yc), want, right in zip(C.CORNERS, (75.0, 75.0, 0.0, 0.0), (0, 0, 1, 1)):
        p, y = np.array([[pc]], dtype=np.float32), np.array([[yc]], dtype=np.float32)
        loss, d, hits, cell_hits = run_kernel(p, y, w1, reduction)
        t_loss, t_grad = torch_f32(p, y, w1, reduction)
        # torch takes log1p(-p) where the kernel takes log(1 - p): its term for p = 1e-30 is 1e-30 w, the kernel's an exact zero
        assert float(loss) == want and abs(t_loss - want) <= 1e-29, (pc, yc, float(loss), t_loss)
        assert ulps(float(d[0, 0]), t_grad[0, 0]) <= 1, (pc, yc, float(d[0, 0]), t_grad)
        assert hits.tolist() == [right, 0] and cell_hits.tolist() == [right]
    p = np.array([c[0] for c in C.CORNERS], dtype=np.float32).reshape(2, 2)
    y = np.array([c[1] for c in C.CORNERS], dtype=np.float32).reshape(2, 2)
    for w in (None, np.array([0.75, 1.5], dtype=np.float32)):
        loss, d, _, _ = run_kernel(p, y, w, reduction)
        t_loss, t_grad = torch_f32(p, y, w, reduction)
        assert float(loss) == t_loss, (float(loss), t_loss)
        assert max(ulps(a, b) for a, b in zip(d.cpu().numpy().ravel(), t_grad.ravel())) <= 1, (d, t_grad)


def test_bad_cells_are_counted_and_never_logged():
    """Targets -0.1, 1.5 and NaN and p = 1.2: NaN loss, four bad cells, exact zeros there, every other cell bit-equal to the clean
    run under "sum". A NaN in p under a good target: NaN loss, NaN in that cell only, not a bad cell."""
    p, y = C.make_case(257, 65, 730)
    w = C.make_weights(65)
    _, d_clean, hits_clean, _ = run_kernel(p, y, w, "sum")
    pb, yb = p.copy(), y.copy()
    cells = [(0, 3), (1, 64), (130, 10), (256, 0)]
    yb[0, 3], yb[1, 64], yb[130, 10], pb[256, 0] = -0.1, 1.5, np.nan, 1.2
    keep = torch.ones(p.shape, dtype=torch.bool)
    for r, k in cells:
        keep[r, k] = False
    for reduction in ("sum", "mean"):
        loss, d, hits, cell_hits = run_kernel(pb, yb, w, reduction)
        ref = C.restated(pb, yb, w, reduction)
        assert bool(torch.isnan(loss)) and hits.tolist() + cell_hits.tolist() == ref["counts"] and int(hits[1]) == 4
        assert not bool(d.cpu()[~keep].any()) and not bool(torch.signbit(d.cpu()[~keep]).any())
        if reduction == "sum":
            assert torch.equal(d.cpu()[keep], d_clean.cpu()[keep])
    with pytest.raises(ValueError, match="4 bad cell"):
        ops.raise_on_bad_targets(hits)
    with pytest.raises(ValueError):
        ops.check_targets(torch.from_numpy(yb), 65)
    ops.check_targets(torch.from_numpy(yb).cuda(), 65)            # device targets are left to the kernel's counter
    pn = p.copy()
    pn[2, 7] = np.nan
    loss, d, hits, _ = run_kernel(pn, y, w, "sum")
    keep = torch.ones(p.shape, dtype=torch.bool)
    keep[2, 7] = False
    assert bool(torch.isnan(loss)) and int(hits[1]) == 0 and bool(torch.isnan(d[2, 7]))
    assert torch.equal(d.cpu()[keep], d_clean.cpu()[keep])


def test_counters_threshold_both_sides_at_one_half():
    from test_bce_cpu import counter_case
    p, y = counter_case()
    ref = C.restated(p, y, None, "mean")
    _, _, hits, cell_hits = run_kernel(p, y, None, "mean")
    assert hits.tolist() + cell_hits.tolist() == ref["counts"] and ref["counts"][0] >= 3


def test_two_runs_are_bit_equal():
    p, y = C.make_case(257, 527, 740)
    w = C.make_weights(527)
    a, b = run_kernel(p, y, w, "mean"), run_kernel(p, y, w, "mean")
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert bool(torch.isfinite(a[0])) and bool(a[1].any())


# ------------------------------------------------------------------ the step -----------------------------------------------------

def vggish(mk, W, ordinals=None):
    torch.manual_seed(77)                                        # Dropout reads the seed at construction
    ens = M.Ensemble("repeat", dict(mk.CNN_CONF), [2, 1], torch.device("cuda"), precision="f32")
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(7, W.ensemble_shapes((2, 1), False)).items()})
    ens.cuda()
    drops = [m for m in ens.mla.modules() if type(m).__name__ == "Dropout"]
    if ordinals is not None:
        for d, o in zip(drops, ordinals):
            d.ordinal = o
    return ens, [d.ordinal for d in drops]


def install(ens, masks):
    for lvl, em in enumerate(ens.mla.embedded_mappings):
        for j, d in enumerate(em.dropouts):
            d.mask = masks["mla.embedded_mappings.%d.dropouts.%d" % (lvl, j)]


def subset_hits(out, y):
    return int(((out >= 0.5) == (y >= 0.5)).all(dim=1).sum())


def test_step_against_torch_autograd_with_the_same_criterion(mk, W):
    """The golden head ([2, 1], f32, injected dropout masks), 8 bags, three steps, BCELoss(weight=linspace(0.5, 2, 10)) on 8 x 10
    multi-hot targets with a few soft entries: against the oracle's model under torch autograd (float64) with that criterion and
    torch.optim.Adam. Tolerances: those of test_step_against_torch_autograd_with_the_same_criterion in tests/test_ce_opts_gpu.py:
    losses rtol 5e-5 (atol 1e-6), parameters rtol 5e-3 (running_var 2e-2) with atol 4e-3 (running_mean 1e-2), the zero-gradient
    biases left out. hits[0] is the subset-accuracy count of the twin's outputs; last_cell_hits its count of cells. The test prints
    the worst ratio per tensor. Measured on the MI355X: every tensor fits, worst ratio 0.194 (embedded_mappings.0.fc.1.weight,
    |p - p_torch| 8.0e-4), then 0.186 (embedded_mappings.1.fc.0.weight, 7.5e-4) and 0.165 (attention_modules.0.normv.bias, 6.6e-4);
    below 0.03 for every other tensor."""
    from oracle import model as omodel
    st = omodel.TrainState(W.make_state_dict(7, W.ensemble_shapes((2, 1), False)), (2, 1), False, False, lr=1e-3)
    for k, v in list(st.sd.items()):
        if v.is_floating_point():
            st.sd[k] = v.detach().double().requires_grad_(v.requires_grad)
    st.opt = torch.optim.Adam([st.sd[k] for k in st.keys], lr=1e-3)
    crit = worker.criterion().double()
    ens, _ = vggish(mk, W)
    step = TR.TrainStep(ens, lr=1e-3, criterion=worker.criterion(), graph=False)
    got, want = [], []
    for s in range(3):
        x, _ = mk.synth_bags(100 + s, 8)
        y = worker.targets(100 + s, 8)
        assert ((y > 0) & (y < 1)).any() and (y == 1).any() and (y == 0).any()
        masks = mk.make_masks(200 + s, [2, 1], 8)
        install(ens, masks)
        labels = (y, y.cuda(), y.double())[s]                     # host, device and float64 targets
        loss, hits = step(x.cuda(), labels)
        got.append(float(loss))
        assert step.last_counted is None and int(hits[1]) == 0
        st.opt.zero_grad()
        stats = {}
        out = omodel.ensemble_forward(st.sd, x.double(), st.model_conf, st.jb, train=True, masks=masks, stats_out=stats)
        ref = crit(out, y.double())
        ref.backward()
        st.opt.step()
        with torch.no_grad():
            omodel.apply_running_stats(st.sd, stats)
        want.append(float(ref.detach()))
        assert int(hits[0]) == subset_hits(out.detach(), y.double())
        assert int(step.last_cell_hits) == int(((out.detach() >= 0.5) == (y.double() >= 0.5)).sum())
    print("losses", got, "torch", want)
    np.testing.assert_allclose(got, want, rtol=5e-5, atol=1e-6)
    sd = ens.state_dict()
    failed = []
    for k, v in st.sd.items():
        if k.startswith("mla.") and "num_batches" not in k and not k.endswith(NOISY):
            atol = 1e-2 if k.endswith("running_mean") else 4e-3
            rtol = 2e-2 if k.endswith("running_var") else 5e-3
            a, b = sd[k].double().cpu().numpy(), v.detach().numpy()
            ratio = float((np.abs(a - b) / (atol + rtol * np.abs(b))).max())
            print("MEASURE %s: worst |p - p_torch| / (atol + rtol |p_torch|) = %.3f, worst |p - p_torch| = %.3g" % (k, ratio, np.abs(a - b).max()))
            if ratio > 1.0:
                failed.append((k, ratio))
    assert not failed, failed
    with pytest.raises(ValueError, match="outside"):
        step(x.cuda(), y * 2)
    with pytest.raises(ValueError, match="shape"):
        step(x.cuda(), torch.zeros(8, dtype=torch.int64))
    with pytest.raises(TypeError):
        TR.TrainStep(ens, criterion=torch.nn.BCEWithLogitsLoss())


def test_eager_steps_equal_graph_replays_with_the_criterion(mk, W):
    runs, ords = {}, None
    for graph in (False, True):
        ens, ords = vggish(mk, W, ordinals=ords)
        crit = worker.criterion()
        step = TR.TrainStep(ens, lr=1e-3, criterion=crit, graph=graph)
        trace = []
        for s in range(4):
            x, _ = mk.synth_bags(300 + s, 8)
            y = worker.targets(300 + s, 8)
            loss, hits = step(x.cuda(), y.cuda() if s % 2 else y.bool() if s == 2 else y)
            trace.append((float(loss), hits.tolist(), int(step.last_cell_hits)))
        runs[graph] = (trace, step, crit)
    (ref, step_e, _), (got, step_g, crit) = runs[False], runs[True]
    assert got == ref, (got, ref)
    assert all(np.isfinite(t[0]) and 0 < t[2] <= 80 for t in got)
    assert step_e._graph is None and step_g._graph is not None and step_g.captures == 1
    assert step_g._graph["y"].dtype == torch.float32 and tuple(step_g._graph["y"].shape) == (8, 10)
    assert any(t is step_g._crit_weight for t in step_g._graph["held"])
    for k in ("flat_p", "flat_m", "flat_v"):
        assert torch.equal(getattr(step_g, k), getattr(step_e, k)), k
    crit.reduction = "sum"
    x, _ = mk.synth_bags(304, 8)
    with pytest.raises(RuntimeError, match="build a new TrainStep"):
        step_g(x.cuda(), worker.targets(304, 8).cuda())


def wide(mk, W, classes, ordinals=None):
    torch.manual_seed(77)
    shapes = W.mla_shapes([2, 1], 128, prefix="mla.", K=classes)
    shapes.update(W.vggish_shapes("cnn.cnn_model."))
    ens = M.Ensemble("repeat", dict(mk.CNN_CONF), [2, 1], torch.device("cuda"), classes=classes)
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(7, shapes).items()})
    ens.cuda()
    drops = [m for m in ens.mla.modules() if type(m).__name__ == "Dropout"]
    if ordinals is not None:
        for d, o in zip(drops, ordinals):
            d.ordinal = o
    return ens, [d.ordinal for d in drops]


def test_wide_heads_train_with_the_criterion(mk, W):
    """classes=20, past the 16-class switch to the wide pooling kernels: two steps, eager and as a graph, finite and bit-equal.
    classes=527 (the AudioSet head): one eager step, finite, no bad cell."""
    runs, ords = [], None
    for graph in (False, True):
        ens, ords = wide(mk, W, 20, ords)
        step = TR.TrainStep(ens, lr=1e-3, criterion=torch.nn.BCELoss(), graph=graph)
        trace = []
        for s in range(2):
            x, _ = mk.synth_bags(400 + s, 4)
            loss, hits = step(x.cuda(), worker.targets(400 + s, 4, K=20).cuda())
            trace.append((float(loss), hits.tolist(), int(step.last_cell_hits)))
        assert (step._graph is not None) == graph
        runs.append((trace, step.flat_p.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert all(np.isfinite(t[0]) and t[1][1] == 0 for t in runs[0][0])
    ens, _ = wide(mk, W, 527)
    step = TR.TrainStep(ens, lr=1e-3, criterion=torch.nn.BCELoss(), graph=False)
    x, _ = mk.synth_bags(402, 4)
    loss, hits = step(x.cuda(), worker.targets(402, 4, K=527, soft=40))
    assert np.isfinite(float(loss)) and int(hits[1]) == 0 and 0 < int(step.last_cell_hits) <= 4 * 527
    assert bool(torch.isfinite(step.flat_p).all())


def test_two_ranks_equal_one_process_on_the_global_batch(tmp_path):
    """Two gloo ranks on one GPU against one process on the global batch of 8: the mean's scale is 1 / (8 x 10) on both ranks, the
    losses and both counters are summed. The ranks are bit-equal to each other; against the one process the tolerances are those
    of tests/test_ce_opts_gpu.py's 2-rank test, with the same tensors left out (the zero-gradient biases and normv.bias)."""
    from test_train_gpu import free_port
    steps, B = 4, 8
    out = str(tmp_path / "dp")
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_bce_dp_worker.py"), out, str(steps), str(B)],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    r0, r1 = np.load(out + ".rank0.npz"), np.load(out + ".rank1.npz")
    one = worker.run(steps, B, 0, B, None)
    for k in r0.files:
        np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)          # replicas stay bit-identical
    np.testing.assert_array_equal(r0["hits"], one["hits"])
    np.testing.assert_array_equal(r0["cell_hits"], one["cell_hits"])
    np.testing.assert_allclose(r0["losses"][:3], one["losses"][:3], rtol=2e-5, atol=1e-6)
    for k in r0.files:
        if k.startswith("mla.") and "num_batches" not in k and not k.endswith(NOISY + ("normv.bias",)):
            np.testing.assert_allclose(r0[k], one[k], rtol=1e-3, atol=1e-2 if k.endswith("running_mean") else 2e-4, err_msg=k)


def test_train_model_with_the_criterion(mk, W, tmp_path):
    """Two epochs over 16 bags: the history holds the validation mAP of multilabel_summary on the collected outputs, the test
    phase returns (mAP, summary), the validation loss is torch's BCELoss on the eval outputs; without extended_criterion the
    TypeError remains."""
    from torch.utils.data import DataLoader, TensorDataset
    x, _ = mk.synth_bags(5, 16)
    y = worker.targets(5, 16)
    ds = TensorDataset(torch.as_tensor(x), y)
    loaders = lambda: {"train": DataLoader(ds, batch_size=8), "val": DataLoader(ds, batch_size=8), "test": DataLoader(ds, batch_size=8)}   # noqa: E731
    ens, _ = vggish(mk, W)
    crit = worker.criterion()
    opt = torch.optim.Adam(TR.trainable_params(ens, True), lr=1e-3)
    before = ens.mla.fc.weight.detach().clone()
    seen = []
    real = TR.multilabel_summary
    TR.multilabel_summary = lambda t, s, names=None: (lambda r: (seen.append((np.array(t), np.array(s), r)), r)[1])(real(t, s, names))
    try:
        out, hist, tested = TR.train_model(ens, loaders(), crit, opt, num_epochs=2, patience=None, save_model_path=str(tmp_path / "m.pt"),
                                           extended_criterion=True)
    finally:
        TR.multilabel_summary = real
    assert len(seen) == 3 and all(t.shape == (16, 10) and s.shape == (16, 10) for t, s, _ in seen)
    assert hist == [seen[0][2]["mAP"], seen[1][2]["mAP"]] and all(0.0 < h <= 1.0 for h in hist)
    assert np.array_equal(seen[0][0], y.numpy()) and seen[0][1].min() > 0.0 and seen[0][1].max() < 1.0
    assert isinstance(tested, tuple) and tested[0] == seen[2][2]["mAP"] and tested[1] is seen[2][2]
    assert tested[1]["classes_without_positives"] == int((y.numpy() < 0.5).all(axis=0).sum())
    ckpt = torch.load(str(tmp_path / "m.pt"), weights_only=True)
    assert ckpt["accuracy"] == max(hist) and ckpt["history"] == hist[:ckpt["epoch"] + 1]
    assert not torch.equal(out.mla.fc.weight.detach(), before) and not opt.state
    v_loss, v_acc, v_out, v_true = TR._evaluate(out, loaders()["val"], torch.device("cuda"), collect=True, criterion=crit)
    assert TR.multilabel_summary(v_true.numpy(), v_out.numpy())["mAP"] == max(hist), "the best-validation weights are restored"
    out.eval()
    want, right = 0.0, 0
    with torch.no_grad():
        for xb, yb in loaders()["val"]:
            scores = out(xb.cuda().float()).cpu()
            want += float(crit(scores, yb)) * xb.shape[0]
            right += subset_hits(scores, yb)
    np.testing.assert_allclose(v_loss, want / 16, rtol=1e-5)
    assert v_acc == right / 16 and tuple(v_out.shape) == (16, 10) and torch.equal(v_true, y)
    ens2, _ = vggish(mk, W)
    with pytest.raises(TypeError):
        TR.train_model(ens2, loaders(), crit, torch.optim.Adam(TR.trainable_params(ens2, True), lr=1e-3), num_epochs=1, patience=None,
                       save_model_path=str(tmp_path / "n.pt"))
