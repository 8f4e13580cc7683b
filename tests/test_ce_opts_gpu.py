"""The criterion options on the GPU (mla_cross_entropy_den / mla_cross_entropy_opts; ops.cross_entropy_opts; TrainStep(criterion=);
train_model(extended_criterion=True)): the kernels against the float64 restatement of tests/ce_opts_cases.py and against the
plain kernel, bad labels, determinism, the step against torch autograd with the same criterion, eager against graph replays, two
data-parallel ranks and the epoch loop."""

import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ce_opts_cases as C
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

ops = importlib.import_module(PKG + ".ops")
M = importlib.import_module(PKG + ".model")
TR = importlib.import_module(PKG + ".train")

NOISY = ("fc.bias", "fc.0.bias", "fc.1.bias", "fcv.bias")     # zero-gradient biases: see test_oracle_golden.py


def strided(t, left=2, right=1):
    """The same values as a column slice of a wider CUDA tensor (pitch = cols + left + right); the rest holds a value that would
    wreck any sum it entered."""
    buf = torch.full((t.shape[0], t.shape[1] + left + right), 1e30, dtype=t.dtype, device="cuda")
    view = buf[:, left:left + t.shape[1]]
    view.copy_(t)
    return view


def run_kernel(x, y, w, ignore_index, eps, reduction, want_grad=True):
    wd = None if w is None else torch.from_numpy(w).cuda()
    loss, d, hits, counted = ops.cross_entropy_opts(strided(torch.from_numpy(x)), torch.from_numpy(y).cuda(), wd, ignore_index, eps, reduction,
                                                    want_grad=want_grad)
    return loss, d, hits, counted


# ------------------------------------------------------------------ the kernels --------------------------------------------------

@pytest.mark.parametrize("rows,K", C.GPU_SHAPES)
def test_kernel_against_the_float64_restatement(rows, K):
    """One wavefront per row, four rows per workgroup, lanes striding over K: K below, at and above one stride and at 16 strides;
    fewer rows than a workgroup holds, exactly four, one more, many. Scores are a column slice of a wider tensor, ties of the row
    maximum are planted (the first index is the prediction), 257 x 10 spreads the logits over +-80, a quarter of the rows are
    ignored (row 0 and the last among them; with one row none, the batch would be all ignored). Options: {no weights, weights
    0.25 .. 4 with one zero} x smoothing {0, 0.1} x {mean, sum}.
    Bounds: MEASURED["cross_entropy loss"] = 2.89e-7 (relative to max(|loss|, 1)) and MEASURED["cross_entropy dscores"] = 1.50e-5
    (max error over max|reference|) of tests/test_train_kernels_gpu.py. Observed maxima over all cases on the MI355X: loss 1.61e-7
    (4 x 10), dscores 3.86e-6 (257 x 10, the +-80 logits; 1.6e-7 at most elsewhere)."""
    b_loss, b_dx = C.bounds()
    x, y = C.make_case(rows, K, 700 + rows + K, spread=C.spread_of(rows, K))
    w = C.make_weights(K)
    ignored = y == -100
    assert rows < 3 or (ignored[0] and ignored[-1] and ignored.sum() >= rows // 4)
    worst = [0.0, 0.0]
    for weighted, eps, reduction in C.OPTIONS:
        wk = w if weighted else None
        ref = C.restated(x, y, wk, -100, eps, reduction)
        loss, d, hits, counted = run_kernel(x, y, wk, -100, eps, reduction)
        assert d.is_contiguous() and tuple(d.shape) == (rows, K)
        d = d.cpu().numpy()
        # K = 1: the gradient is exactly zero (asserted below); the float64 restatement leaves a rounding residue to divide by
        e_loss, e_dx = C.loss_err(float(loss), ref["loss"]), C.rel(d, ref["dx"]) if K > 1 else 0.0
        worst = [max(worst[0], e_loss), max(worst[1], e_dx)]
        print("%d x %d weights %s smoothing %g %s: loss error %.3g (bound %.3g), dscores error %.3g (bound %.3g)"
              % (rows, K, weighted, eps, reduction, e_loss, b_loss, e_dx, b_dx))
        assert e_loss < b_loss and e_dx < b_dx, (weighted, eps, reduction, e_loss, e_dx)
        assert hits.tolist() + counted.tolist() == ref["counts"]
        assert ops.raise_on_bad_labels(hits) == ref["counts"][0]
        assert not d[ignored].any() and not np.signbit(d[ignored]).any(), "ignored rows are stored as exact zeros"
        if K == 1:
            assert float(loss) == 0.0 and not d.any()
        loss2, d2, hits2, counted2 = run_kernel(x, y, wk, -100, eps, reduction, want_grad=False)
        assert d2 is None and torch.equal(loss2, loss) and torch.equal(hits2, hits) and torch.equal(counted2, counted)
    print("%d x %d: worst loss error %.3g, worst dscores error %.3g" % (rows, K, worst[0], worst[1]))


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_all_rows_ignored_and_an_ignored_class(reduction):
    x, _ = C.make_case(6, 65, 710)
    w = C.make_weights(65)
    loss, d, hits, counted = run_kernel(x, np.full(6, -100, dtype=np.int64), w, -100, 0.1, reduction)
    assert (bool(torch.isnan(loss)) if reduction == "mean" else float(loss) == 0.0) and not bool(d.any())
    assert hits.tolist() == [0, 0] and counted.tolist() == [0]
    y3 = np.array([3, 1, 3, 64, 0, 3], dtype=np.int64)
    ref = C.restated(x, y3, w, 3, 0.1, reduction)
    loss, d, hits, counted = run_kernel(x, y3, w, 3, 0.1, reduction)
    b_loss, b_dx = C.bounds()
    assert C.loss_err(float(loss), ref["loss"]) < b_loss and C.rel(d.cpu().numpy(), ref["dx"]) < b_dx
    assert hits.tolist() + counted.tolist() == ref["counts"] and counted.tolist() == [3] and not bool(d[[0, 2, 5]].any())


@pytest.mark.parametrize("rows,K", [(257, 10), (5, 65), (256, 527)])
def test_plain_options_equal_the_old_kernel(rows, K):
    """No weight, no smoothing, mean, no ignored row: the same hits as ops.cross_entropy; loss and dscores within twice the bound
    (each lies within it of float64)."""
    b_loss, b_dx = C.bounds()
    x, y = C.make_case(rows, K, 720 + rows, ignore=False)
    xs, yd = strided(torch.from_numpy(x)), torch.from_numpy(y).cuda()
    loss0, d0, hits0 = ops.cross_entropy(xs, yd, 1.0 / rows)
    loss, d, hits, counted = ops.cross_entropy_opts(xs, yd)
    assert torch.equal(hits, hits0) and counted.tolist() == [rows]
    e_loss, e_dx = C.loss_err(float(loss), float(loss0)), C.rel(d.cpu().numpy(), d0.cpu().numpy())
    print("plain %d x %d: |loss - old| %.3g (bound %.3g), dscores %.3g (bound %.3g)" % (rows, K, e_loss, 2 * b_loss, e_dx, 2 * b_dx))
    assert e_loss < 2 * b_loss and e_dx < 2 * b_dx


@pytest.mark.parametrize("rows,K", [(257, 10), (5, 2)])
def test_bad_labels_are_counted_and_never_used(rows, K):
    """The case of test_cross_entropy_refuses_labels_outside_the_classes with -100 now ignored: -1, K and 2**40 are bad. NaN loss,
    n_bad = 3, zero rows for the four, every other row bit-equal to the clean run."""
    x, good = C.make_case(rows, K, 730 + rows, ignore=False)
    w = C.make_weights(K)
    bad = {0: -1, rows // 2: K, rows - 1: -100, 3: 2 ** 40}
    y = good.copy()
    for r, v in bad.items():
        y[r] = v
    _, d_good, hits_good, _ = run_kernel(x, good, w, -100, 0.1, "sum")
    loss, d, hits, counted = run_kernel(x, y, w, -100, 0.1, "sum")
    assert bool(torch.isnan(loss)) and int(hits[1]) == 3 and counted.tolist() == [rows - 1]
    keep = torch.ones(rows, dtype=torch.bool)
    keep[list(bad)] = False
    assert not bool(d.cpu()[~keep].any()) and torch.equal(d.cpu()[keep], d_good.cpu()[keep])
    assert int(hits[0]) == int(((np.argmax(x, axis=1) == good) & keep.numpy()).sum())
    with pytest.raises(IndexError):
        ops.raise_on_bad_labels(hits)
    with pytest.raises(IndexError):
        ops.check_labels_ignoring(torch.from_numpy(y), K, -100)


def test_two_runs_are_bit_equal():
    x, y = C.make_case(257, 527, 740)
    w = C.make_weights(527)
    a, b = run_kernel(x, y, w, -100, 0.1, "mean"), run_kernel(x, y, w, -100, 0.1, "mean")
    assert all(torch.equal(p, q) for p, q in zip(a, b))
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


def weighted_criterion(**kw):
    return torch.nn.CrossEntropyLoss(weight=torch.linspace(0.5, 2.0, 10), label_smoothing=0.1, **kw)


def bags(mk, seed, B, ignored=(1, 5)):
    x, y = mk.synth_bags(seed, B)
    y = y.clone()
    y[list(ignored)] = -100
    return x, y


def test_step_against_torch_autograd_with_the_same_criterion(mk, W):
    """The golden head ([2, 1], f32, injected dropout masks), 8 bags, three steps, two labels -100, CrossEntropyLoss(weight,
    label_smoothing=0.1): against the oracle's model under torch autograd (float64) with that criterion and torch.optim.Adam.
    Tolerances: those of the plain step's own comparison with a run of the reference after a few head-only Adam steps,
    tests/test_train_gpu.py test_step_updates_exactly_what_the_optimizer_holds: losses rtol 5e-5 (atol 1e-6) on the first steps,
    parameters rtol 5e-3 (running_var 2e-2) with atol 4e-3 (running_mean 1e-2), its zero-gradient biases left out. Adam turns a
    gradient entry that is rounding noise into a step of up to +-lr, so a third of the 360 000 entries of
    embedded_mappings.0.fc.1.weight (|g| < 1e-7 in float64) are pinned no tighter than that. Measured on the MI355X, worst
    |p - p_torch| after the three steps: 5.3e-4 (embedded_mappings.1.fc.0.weight), 4.8e-4 (embedded_mappings.0.fc.1.weight), below
    2.5e-5 for every other tensor; losses agree to 1.3e-6 relative. torch's own float32 run lies 2.6e-4 and 1.5e-4 from its
    float64 run on those two tensors.
    And criterion=None is TrainStep() itself: bit-equal loss and parameters."""
    from oracle import model as omodel
    st = omodel.TrainState(W.make_state_dict(7, W.ensemble_shapes((2, 1), False)), (2, 1), False, False, lr=1e-3)
    for k, v in list(st.sd.items()):
        if v.is_floating_point():
            st.sd[k] = v.detach().double().requires_grad_(v.requires_grad)
    st.opt = torch.optim.Adam([st.sd[k] for k in st.keys], lr=1e-3)
    crit = weighted_criterion().double()
    ens, _ = vggish(mk, W)
    step = TR.TrainStep(ens, lr=1e-3, criterion=weighted_criterion(), graph=False)
    got, want = [], []
    for s in range(3):
        x, y = bags(mk, 100 + s, 8)
        masks = mk.make_masks(200 + s, [2, 1], 8)
        install(ens, masks)
        loss, hits = step(x.cuda(), y)
        got.append(float(loss))
        assert int(step.last_counted) == 6 and int(hits[1]) == 0
        st.opt.zero_grad()
        stats = {}
        out = omodel.ensemble_forward(st.sd, x.double(), st.model_conf, st.jb, train=True, masks=masks, stats_out=stats)
        ref = crit(out, y)
        ref.backward()
        st.opt.step()
        with torch.no_grad():
            omodel.apply_running_stats(st.sd, stats)
        want.append(float(ref.detach()))
        keep = y != -100
        assert int(hits[0]) == int((out.detach().argmax(dim=1)[keep] == y[keep]).sum())
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
            print("%s: worst |p - p_torch| / (atol + rtol |p_torch|) = %.3f" % (k, ratio))
            if ratio > 1.0:
                failed.append((k, ratio))
    assert not failed, failed
    runs = []
    for kw in ({}, {"criterion": None}):
        ens, _ = vggish(mk, W)
        step = TR.TrainStep(ens, lr=1e-3, graph=False, **kw)
        losses = []
        for s in range(2):
            x, y = mk.synth_bags(100 + s, 8)
            install(ens, mk.make_masks(200 + s, [2, 1], 8))
            losses.append(float(step(x.cuda(), y.cuda())[0]))
        assert step.last_counted is None
        runs.append((losses, step.flat_p.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


def test_eager_steps_equal_graph_replays_with_the_criterion(mk, W):
    runs, ords = {}, None
    for graph in (False, True):
        ens, ords = vggish(mk, W, ordinals=ords)
        crit = weighted_criterion()
        step = TR.TrainStep(ens, lr=1e-3, criterion=crit, graph=graph)
        trace = []
        for s in range(4):
            x, y = bags(mk, 300 + s, 8, ignored=(s, 7))
            loss, hits = step(x.cuda(), y.cuda())
            trace.append((float(loss), hits.tolist(), int(step.last_counted)))
        runs[graph] = (trace, step, crit)
    (ref, step_e, _), (got, step_g, crit) = runs[False], runs[True]
    assert got == ref, (got, ref)
    assert all(t[2] == 6 for t in got)
    assert step_e._graph is None and step_g._graph is not None and step_g.captures == 1
    for k in ("flat_p", "flat_m", "flat_v"):
        assert torch.equal(getattr(step_g, k), getattr(step_e, k)), k
    crit.label_smoothing = 0.2
    x, y = bags(mk, 304, 8)
    with pytest.raises(RuntimeError, match="build a new TrainStep"):
        step_g(x.cuda(), y.cuda())


def test_two_ranks_equal_one_process_on_the_global_batch(tmp_path):
    """Two gloo ranks on one GPU, weights and smoothing, ignored rows split three to one: the denominator is the global batch's,
    so both ranks and the one-process run agree. Tolerances: those of tests/test_adam_groups_gpu.py's 2-rank test (the ranks'
    float32 partial denominators may differ from the one-process one by one unit in the last place). Left out: the zero-gradient
    biases tests/test_train_gpu.py leaves out (NOISY: a Linear bias in front of a BatchNorm; mla.fc.bias came out up to 3.1e-3
    apart after four steps) and, for the same reason, the attention modules' normv.bias. It shifts all classes of a time
    slot alike and the softmax over the classes cancels the shift, so its gradient is zero in exact arithmetic and rounding noise
    in float32, which Adam turns into steps of up to +-lr that follow the summation order (two ranks against one process:
    2 of 10 entries 2.8e-4 apart after four steps; the ranks themselves stay bit-equal, normv.bias included)."""
    from test_train_gpu import free_port
    import _ce_opts_dp_worker as worker
    steps, B = 4, 8
    out = str(tmp_path / "dp")
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_ce_opts_dp_worker.py"), out, str(steps), str(B)],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    r0, r1 = np.load(out + ".rank0.npz"), np.load(out + ".rank1.npz")
    one = worker.run(steps, B, 0, B, None)
    for k in r0.files:
        np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)          # replicas stay bit-identical
    assert r0["counted"].tolist() == one["counted"].tolist() == [B - len(worker.IGNORED)] * steps
    np.testing.assert_array_equal(r0["hits"], one["hits"])
    np.testing.assert_allclose(r0["losses"][:3], one["losses"][:3], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(r0["losses"], one["losses"], rtol=2e-3, atol=1e-5)
    for k in r0.files:
        if k.startswith("mla.") and "num_batches" not in k and not k.endswith(NOISY + ("normv.bias",)):
            np.testing.assert_allclose(r0[k], one[k], rtol=1e-3, atol=1e-2 if k.endswith("running_mean") else 2e-4, err_msg=k)


def test_train_model_with_the_extended_criterion(mk, W, tmp_path):
    """Two epochs over 16 bags with a -100 label in the train, val and test splits: runs to the end, the validation loss is
    torch's criterion on the eval outputs, the accuracy divides by all rows; without extended_criterion the label raises."""
    from torch.utils.data import DataLoader, TensorDataset
    x, y = bags(mk, 5, 16, ignored=(2, 11))
    ds = TensorDataset(torch.as_tensor(x), torch.as_tensor(y))
    loaders = lambda: {"train": DataLoader(ds, batch_size=8), "val": DataLoader(ds, batch_size=8), "test": DataLoader(ds, batch_size=8)}   # noqa: E731
    ens, _ = vggish(mk, W)
    crit = weighted_criterion()
    opt = torch.optim.Adam(TR.trainable_params(ens, True), lr=1e-3)
    before = ens.mla.fc.weight.detach().clone()
    seen = []
    real_eval = TR._evaluate
    TR._evaluate = lambda *a, **k: (lambda r: (seen.append((k.get("criterion"), r[0])), (r[0], 0.5 + 0.1 * len(seen)) + tuple(r[2:]))[1])(real_eval(*a, **k))
    try:
        out, hist, tested = TR.train_model(ens, loaders(), crit, opt, num_epochs=2, patience=None, save_model_path=str(tmp_path / "m.pt"),
                                           extended_criterion=True)
    finally:
        TR._evaluate = real_eval
    assert len(hist) == 2 and all(c is crit for c, _ in seen) and all(np.isfinite(v) for _, v in seen)
    assert isinstance(tested, tuple) and tested[1]["macro avg"]["support"] == 14, "ignored rows are left out of the summary"
    assert not torch.equal(out.mla.fc.weight.detach(), before) and not opt.state
    v_loss, v_acc = TR._evaluate(out, loaders()["val"], torch.device("cuda"), criterion=crit)
    out.eval()
    want, right = 0.0, 0
    with torch.no_grad():
        for xb, yb in loaders()["val"]:
            scores = out(xb.cuda().float()).cpu()
            want += float(crit(scores, yb)) * xb.shape[0]
            right += int((scores.argmax(dim=1) == yb).sum())
    np.testing.assert_allclose(v_loss, want / 16, rtol=1e-5)
    assert v_acc == right / 16
    ens2, _ = vggish(mk, W)
    with pytest.raises(IndexError):
        TR.train_model(ens2, loaders(), crit, torch.optim.Adam(TR.trainable_params(ens2, True), lr=1e-3), num_epochs=1, patience=None,
                       save_model_path=str(tmp_path / "n.pt"))
