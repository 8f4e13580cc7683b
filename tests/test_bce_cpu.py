"""The binary cross-entropy without a GPU: the float64 restatement of tests/bce_cases.py against torch's own binary_cross_entropy
in float64; the kernels' work simulated on the host (csrc/bce_hostsim.cpp runs csrc/bce_core.h lane by lane in the kernels' order,
in float32) against the restatement under the bounds the GPU test uses, one store per dp element, no read past the operands;
saturation against torch's float32 result; bad cells and NaN; the counters; the C entries' argument errors, reported before any
launch; criterion parsing, the host-side target check, and the mAP / AUC report against a brute-force restatement and sklearn."""

import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bce_cases as C
from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bce_hostsim") / "bce_hostsim.so")
    src = os.path.join(ROOT, PKG, "csrc", "bce_hostsim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, ci, cf = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    lib.hostsim_bce.argtypes = [vp, i64, vp, i64, i64, ci, vp, ci, cf, vp, vp, i64, vp, vp, vp]
    lib.hostsim_bce_workspace_bytes.argtypes = [i64]
    lib.hostsim_bce_workspace_bytes.restype = i64
    return lib


def bounds():
    """(loss, dprobs): the table of tests/test_bce_gpu.py."""
    from test_bce_gpu import MEASURED
    return MEASURED["bce loss"][1], MEASURED["bce dprobs"][1]


# ------------------------------------------------------------------ the restatement against torch ---------------------------

@pytest.mark.parametrize("weighted,reduction", C.OPTIONS)
def test_restatement_equals_torch_in_float64(weighted, reduction):
    p, y = C.make_case(13, 7, 40)
    w = C.make_weights(7) if weighted else None
    ref = C.restated(p, y, w, reduction)
    p64 = torch.from_numpy(p).double().requires_grad_(True)
    loss = F.binary_cross_entropy(p64, torch.from_numpy(y).double(), weight=None if w is None else torch.from_numpy(w).double(),
                                  reduction=reduction)
    loss.backward()
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    assert float(np.abs(ref["dp"] - p64.grad.numpy()).max()) <= 1e-12
    soft = (y > 0) & (y < 1)
    assert 10 <= soft.sum() <= 40 and (y[~soft] == 1).any() and (y[~soft] == 0).any()
    assert ref["counts"] == [int(((p >= 0.5) == (y >= 0.5)).all(axis=1).sum()), 0, int(((p >= 0.5) == (y >= 0.5)).sum())]
    half = C.restated(p, y, w, reduction, inv_total=0.5 / (13 * 7))
    if reduction == "mean":
        assert abs(half["loss"] * 2 - ref["loss"]) <= 1e-15 and np.allclose(half["dp"] * 2, ref["dp"], rtol=0, atol=1e-16)
    else:
        assert half["loss"] == ref["loss"] and np.array_equal(half["dp"], ref["dp"])


# ------------------------------------------------------------------ the kernels on the host ----------------------------------

def run_hostsim(hostsim, p, y, w, reduction, inv_total=None, pad=3, want_grad=True):
    """-> dict like the restatement's. p lies in a buffer of exactly (rows - 1) (K + pad) + K floats and the targets in one with
    a pitch of K + 2: the recorded highest reads must be the last elements. dp comes in NaN-filled with a pitch of K + 1; one
    store per element, none into the padding."""
    rows, K = p.shape
    pb = np.full((rows, K + pad), 1e30, dtype=np.float32)
    pb[:, :K] = p
    yb = np.full((rows, K + 2), 1e30, dtype=np.float32)
    yb[:, :K] = y
    dp = np.full((rows, K + 1), np.nan, dtype=np.float32)
    writes = np.zeros((rows, K + 1), dtype=np.int32)
    loss, counts, max_read = np.zeros(1, dtype=np.float32), np.zeros(3, dtype=np.int32), np.zeros(2, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    scale = 1.0 / (rows * K) if inv_total is None else inv_total
    rc = hostsim.hostsim_bce(ptr(pb), K + pad, ptr(yb), K + 2, rows, K, ptr(w), {"mean": 0, "sum": 1}[reduction], scale, ptr(loss),
                             ptr(dp) if want_grad else None, K + 1, ptr(writes), ptr(counts), ptr(max_read))
    assert rc == 0, rc
    if want_grad:
        assert (writes[:, :K] == 1).all() and not writes[:, K:].any(), "every element of dp is written exactly once"
        assert np.isnan(dp[:, K:]).all()
    else:
        assert not writes.any()
    assert max_read.tolist() == [(rows - 1) * (K + pad) + K - 1, (rows - 1) * (K + 2) + K - 1], "the last element of the last row"
    return {"loss": float(loss[0]), "dp": dp[:, :K].copy(), "counts": counts.tolist()}


@pytest.mark.parametrize("rows,K", C.HOSTSIM_SHAPES)
def test_hostsim_against_the_restatement(hostsim, rows, K):
    b_loss, b_dp = bounds()
    p, y = C.make_case(rows, K, 50 + rows + K)
    w = C.make_weights(K)
    worst = [0.0, 0.0]
    for weighted, reduction in C.OPTIONS:
        wk = w if weighted else None
        ref = C.restated(p, y, wk, reduction)
        got = run_hostsim(hostsim, p, y, wk, reduction)
        e_loss, e_dp = C.loss_err(got["loss"], ref["loss"]), C.rel(got["dp"], ref["dp"])
        worst = [max(worst[0], e_loss), max(worst[1], e_dp)]
        assert e_loss < b_loss and e_dp < b_dp, (weighted, reduction, e_loss, e_dp)
        assert got["counts"] == ref["counts"] and got["counts"][1] == 0
        blind = run_hostsim(hostsim, p, y, wk, reduction, want_grad=False)
        assert np.float32(blind["loss"]).tobytes() == np.float32(got["loss"]).tobytes() and blind["counts"] == got["counts"]
    print("hostsim %d x %d: worst loss error %.3g (bound %.3g), worst dprobs error %.3g (bound %.3g)" % (rows, K, worst[0], b_loss, worst[1], b_dp))


def ulps(a, b):
    """Distance of two float32 values in units in the last place of b."""
    a, b = np.float32(a), np.float32(b)
    if a == b:
        return 0.0
    return abs(float(a) - float(b)) / float(np.spacing(np.abs(b)))


def torch_f32(p, y, w, reduction):
    p32 = torch.tensor(p, dtype=torch.float32).requires_grad_(True)
    loss = F.binary_cross_entropy(p32, torch.tensor(y, dtype=torch.float32), weight=None if w is None else torch.tensor(w), reduction=reduction)
    loss.backward()
    return float(loss.detach()), p32.grad.numpy()


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_saturation_equals_torch_float32(hostsim, reduction):
    """p = 0 with y = 1, p = 1 with y = 0, p = 1 with y = 1, p = 1e-30 with y = 0: the clamps at -100 and 1e-12. Against torch's own
    float32 CPU result for the same inputs: each corner alone (1 x 1: the terms 100 w and 0 are exact) and the four in a 2 x 2 (the
    mean's scale 1 / 4 is exact). These cells stay out of the relative-error cases: a gradient of 1e12 would hide everything else."""
    w1 = np.array([0.75], dtype=np.float32)
    for (pc, yc), want, right in zip(C.CORNERS, (75.0, 75.0, 0.0, 0.0), (0, 0, 1, 1)):
        p, y = np.array([[pc]], dtype=np.float32), np.array([[yc]], dtype=np.float32)
        got = run_hostsim(hostsim, p, y, w1, reduction)
        t_loss, t_grad = torch_f32(p, y, w1, reduction)
        # torch takes log1p(-p) where the kernel takes log(1 - p): its term for p = 1e-30 is 1e-30 w, the kernel's an exact zero
        assert got["loss"] == want and abs(t_loss - want) <= 1e-29, (pc, yc, got["loss"], t_loss)
        assert ulps(got["dp"][0, 0], t_grad[0, 0]) <= 1, (pc, yc, got["dp"], t_grad)
        assert got["counts"] == [right, 0, right]              # the first two corners are as wrong as a cell can be
    p = np.array([c[0] for c in C.CORNERS], dtype=np.float32).reshape(2, 2)
    y = np.array([c[1] for c in C.CORNERS], dtype=np.float32).reshape(2, 2)
    for w in (None, np.array([0.75, 1.5], dtype=np.float32)):
        got = run_hostsim(hostsim, p, y, w, reduction)
        t_loss, t_grad = torch_f32(p, y, w, reduction)
        assert got["loss"] == t_loss, (got["loss"], t_loss)
        assert max(ulps(a, b) for a, b in zip(got["dp"].ravel(), t_grad.ravel())) <= 1, (got["dp"], t_grad)
        assert np.abs(got["dp"][0]).min() >= 1e11 and got["dp"][1, 0] == 0.0


def test_bad_cells_are_counted_and_never_logged(hostsim):
    """Targets -0.1, 1.5 and NaN and p = 1.2: NaN loss, four bad cells, exact zeros there, every other cell bit-equal to the clean
    run. A NaN in p under a good target: NaN loss, NaN in that cell only, not a bad cell."""
    p, y = C.make_case(6, 65, 60)
    w = C.make_weights(65)
    clean = run_hostsim(hostsim, p, y, w, "sum")
    pb, yb = p.copy(), y.copy()
    cells = [(0, 3), (1, 64), (4, 10), (5, 0)]
    yb[0, 3], yb[1, 64], yb[4, 10], pb[5, 0] = -0.1, 1.5, np.nan, 1.2
    for reduction in ("sum", "mean"):
        got = run_hostsim(hostsim, pb, yb, w, reduction)
        ref = C.restated(pb, yb, w, reduction)
        assert np.isnan(got["loss"]) and np.isnan(ref["loss"]) and got["counts"] == ref["counts"] and got["counts"][1] == 4
        for r, k in cells:
            assert got["dp"][r, k] == 0.0 and not np.signbit(got["dp"][r, k])
    got = run_hostsim(hostsim, pb, yb, w, "sum")
    keep = np.ones(p.shape, dtype=bool)
    for r, k in cells:
        keep[r, k] = False
    assert got["dp"][keep].tobytes() == clean["dp"][keep].tobytes()
    assert got["counts"][0] <= clean["counts"][0] and got["counts"][2] <= clean["counts"][2]
    pn = p.copy()
    pn[2, 7] = np.nan
    got = run_hostsim(hostsim, pn, y, w, "sum")
    keep = np.ones(p.shape, dtype=bool)
    keep[2, 7] = False
    assert np.isnan(got["loss"]) and got["counts"][1] == 0 and np.isnan(got["dp"][2, 7])
    assert got["dp"][keep].tobytes() == clean["dp"][keep].tobytes()


def counter_case():
    """9 x 65: rows 0, 4 and 8 are exact matches (p pushed to the side of its target), row 4 through ties: p == 0.5 against y = 1
    and against y == 0.5, both of which count as "at least 0.5"; row 1 misses in one cell only, through p just below 0.5."""
    p, y = C.make_case(9, 65, 70)
    for r in (0, 1, 4, 8):
        p[r] = np.where(y[r] >= 0.5, np.maximum(p[r], 0.6), np.minimum(p[r], 0.4)).astype(np.float32)
    p[4, 0], y[4, 0] = 0.5, 1.0
    p[4, 64], y[4, 64] = 0.5, 0.5
    p[4, 1], y[4, 1] = 0.9, 0.5
    p[1, 64], y[1, 64] = np.nextafter(np.float32(0.5), np.float32(0)), 0.5
    return p, y


def test_counters_threshold_both_sides_at_one_half(hostsim):
    p, y = counter_case()
    ref = C.restated(p, y, None, "mean")
    right = (p >= 0.5) == (y >= 0.5)
    assert right[[0, 4, 8]].all() and right[1].sum() == 64 and ref["counts"][0] >= 3
    assert ref["counts"] == [int(right.all(axis=1).sum()), 0, int(right.sum())]
    got = run_hostsim(hostsim, p, y, C.make_weights(65), "mean")
    assert got["counts"] == ref["counts"]


# ------------------------------------------------------------------ the C entries ---------------------------------------------

def test_argument_errors_are_reported_before_any_launch(L, hostsim):
    lib = L.lib()
    for sym in ("mla_bce", "mla_bce_workspace_bytes"):
        assert sym in L.declared_symbols() and hasattr(lib, sym)
    for rows in (1, 5, 257, 5120):
        assert lib.mla_bce_workspace_bytes(rows) == hostsim.hostsim_bce_workspace_bytes(rows) >= 16 * rows
        assert lib.mla_bce_workspace_bytes(rows) % 8 == 0
    fake = ctypes.c_void_p(0x1000)                       # device pointers: never dereferenced, every call below fails validation first
    E_ARG, E_SHAPE = -1, -2

    def bce(p=fake, ldp=12, target=fake, ldt=10, rows=8, K=10, weight=fake, reduction=0, scale=1.0 / 80, loss=fake, dp=fake, ld_dp=10,
            counts=fake, ws=fake):
        return lib.mla_bce(p, ldp, target, ldt, rows, K, weight, reduction, scale, loss, dp, ld_dp, counts, ws, None)

    def expect(code, rc, needle):
        assert rc == code, (rc, lib.mla_last_error())
        assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    for null in ("p", "target", "loss", "counts", "ws"):
        expect(E_ARG, bce(**{null: None}), "null")
    for rows in (0, -3):
        expect(E_ARG, bce(rows=rows), "rows")
    for K in (0, -1, 1025):
        expect(E_SHAPE, bce(K=K, ldp=2048, ldt=2048, ld_dp=2048), "classes")
    for pitch in ("ldp", "ldt", "ld_dp"):
        expect(E_ARG, bce(**{pitch: 9}), "pitch")
    for code in (-1, 2, 7):
        expect(E_ARG, bce(reduction=code), "reduction")
    for scale in (0.0, -0.5, float("nan"), float("inf")):
        expect(E_ARG, bce(scale=scale), "scale")
    expect(E_ARG, bce(ws=ctypes.c_void_p(0x1004)), "aligned")


# ------------------------------------------------------------------ host logic -------------------------------------------------

def test_criterion_parsing_refuses_what_the_step_cannot_do():
    TR = importlib.import_module(PKG + ".train")
    BCE = torch.nn.BCELoss
    assert TR.parse_bce_criterion(BCE(), 10) == {"weight": None, "reduction": "mean"}
    w = torch.linspace(0.5, 2.0, 10, dtype=torch.float64)
    got = TR.parse_bce_criterion(BCE(weight=w, reduction="sum"), 10)
    assert got["weight"].dtype == torch.float32 and torch.equal(got["weight"], w.float()) and not got["weight"].is_cuda
    assert got["reduction"] == "sum"
    assert TR.parse_bce_criterion(BCE(weight=torch.tensor([0.0, 1.0])), 2)["weight"].tolist() == [0.0, 1.0]      # one zero weight is fine
    with pytest.raises(ValueError, match="scalar"):
        TR.parse_bce_criterion(BCE(reduction="none"), 10)
    for bad in (torch.ones(9), torch.ones(11), torch.ones(2, 5)):
        with pytest.raises(ValueError, match="classes"):
            TR.parse_bce_criterion(BCE(weight=bad), 10)
    neg, nan, inf = torch.ones(10), torch.ones(10), torch.ones(10)
    neg[4], nan[4], inf[4] = -0.5, float("nan"), float("inf")
    for bad in (neg, nan, inf):
        with pytest.raises(ValueError, match="finite and non-negative"):
            TR.parse_bce_criterion(BCE(weight=bad), 10)
    with pytest.raises(ValueError, match="all zero"):
        TR.parse_bce_criterion(BCE(weight=torch.zeros(10)), 10)
    with pytest.raises(ValueError, match="float"):
        TR.parse_bce_criterion(BCE(weight=torch.ones(10, dtype=torch.int64)), 10)
    with pytest.raises(NotImplementedError):
        TR.parse_bce_criterion(BCE(), 1025)
    for other in (torch.nn.BCEWithLogitsLoss(), torch.nn.CrossEntropyLoss(), torch.nn.MSELoss()):
        with pytest.raises(TypeError):
            TR.parse_bce_criterion(other, 10)
    for other in (BCE(), torch.nn.BCEWithLogitsLoss()):                    # the cross-entropy parser knows neither
        with pytest.raises(TypeError):
            TR.parse_criterion(other, 10)


def test_check_targets_and_raise_on_bad_targets():
    ops = importlib.import_module(PKG + ".ops")
    ops.check_targets(torch.tensor([[0.0, 1.0, 0.3], [1.0, 1.0, 0.0]]), 3)
    ops.check_targets(torch.tensor([[0, 1, 1]]), 3)                        # integer and bool multi-hot targets pass
    ops.check_targets(torch.tensor([[True, False, True]]), 3)
    ops.check_targets(torch.zeros((0, 3)), 3)
    for shape in ((4,), (4, 2), (4, 4), (2, 2, 3)):
        with pytest.raises(ValueError, match="shape"):
            ops.check_targets(torch.zeros(shape), 3)
    for bad, needle in ((-0.1, "outside"), (1.5, "outside"), (2, "outside"), (float("nan"), "NaN")):
        with pytest.raises(ValueError, match=needle):
            ops.check_targets(torch.tensor([[0, 1, bad]]), 3)
    assert ops.raise_on_bad_targets(torch.tensor([5, 0], dtype=torch.int32)) == 5
    with pytest.raises(ValueError, match="3 bad cell"):
        ops.raise_on_bad_targets(torch.tensor([5, 3], dtype=torch.int32))


# ------------------------------------------------------------------ the report --------------------------------------------------

def report_fixture():
    """40 x 6, scores quantised to twelfths so that ties occur inside and across the two groups; class 4 has no positive and
    class 5 no negative. A few soft targets (positive at >= 0.5)."""
    rng = np.random.default_rng(90)
    y = (rng.uniform(0, 1, (40, 6)) < 0.35).astype(np.float64)
    y[:, 4], y[:, 5] = 0.0, 1.0
    y[3, 0], y[7, 1], y[9, 2] = 0.5, 0.7, 0.2
    s = np.round((0.35 * (y >= 0.5) + rng.uniform(0, 0.65, (40, 6))) * 12) / 12
    return y, s


def brute_force(t, s):
    """The two definitions written out, O(n^2): AP over the distinct thresholds, AUC as the Mann-Whitney statistic."""
    pos, neg = s[t], s[~t]
    ap = float("nan")
    if len(pos):
        ap, prev = 0.0, 0.0
        for thr in sorted(set(s.tolist()), reverse=True):
            tp, fp = sum(1 for v in pos if v >= thr), sum(1 for v in neg if v >= thr)
            recall = tp / len(pos)
            ap += (recall - prev) * tp / (tp + fp)
            prev = recall
    auc = float("nan")
    if len(pos) and len(neg):
        auc = sum(1.0 if a > b else 0.5 if a == b else 0.0 for a in pos for b in neg) / (len(pos) * len(neg))
    return ap, auc


def test_multilabel_summary_against_the_definitions_and_sklearn():
    TR = importlib.import_module(PKG + ".train")
    y, s = report_fixture()
    names = ["c%d" % i for i in range(6)]
    res = TR.multilabel_summary(y, s, names)
    t = y >= 0.5
    assert any(len(set(s[:, c].tolist())) < 20 for c in range(6)), "ties occur"
    aps, aucs = [], []
    for c, name in enumerate(names):
        ap, auc = brute_force(t[:, c], s[:, c])
        for got, want in ((res[name]["average_precision"], ap), (res[name]["roc_auc"], auc)):
            assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-12, (name, got, want)
        assert res[name]["support"] == int(t[:, c].sum())
        aps.append(ap); aucs.append(auc)
    assert np.isnan(res["c4"]["average_precision"]) and np.isnan(res["c4"]["roc_auc"]) and np.isnan(res["c5"]["roc_auc"])
    assert not np.isnan(res["c5"]["average_precision"])
    assert res["classes_without_positives"] == 1 and res["classes_undefined_auc"] == 2
    assert abs(res["mAP"] - np.nanmean(aps)) <= 1e-12 and abs(res["mAUC"] - np.nanmean(aucs)) <= 1e-12
    want_d = float(np.sqrt(2.0) * torch.special.ndtri(torch.tensor(np.nanmean(aucs), dtype=torch.float64)))
    assert abs(res["d_prime"] - want_d) <= 1e-12 and res["d_prime"] > 0
    pred = s >= 0.5
    assert res["subset_accuracy"] == (pred == t).all(axis=1).mean()
    tp = (pred & t).sum()
    prec, rec = tp / pred.sum(), tp / t.sum()
    micro = res["micro avg"]
    assert abs(micro["precision"] - prec) <= 1e-12 and abs(micro["recall"] - rec) <= 1e-12
    assert abs(micro["f1-score"] - 2 * prec * rec / (prec + rec)) <= 1e-12 and micro["support"] == int(t.sum())
    assert list(TR.multilabel_summary(y, s))[:6] == ["class_%d" % i for i in range(6)]
    with pytest.raises(ValueError):
        TR.multilabel_summary(y, s[:, :5])


def test_multilabel_summary_against_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    TR = importlib.import_module(PKG + ".train")
    y, s = report_fixture()
    res = TR.multilabel_summary(y, s, ["c%d" % i for i in range(6)])
    t = (y >= 0.5).astype(int)
    for c in range(6):
        if t[:, c].any():
            assert abs(res["c%d" % c]["average_precision"] - metrics.average_precision_score(t[:, c], s[:, c])) <= 1e-12
        if t[:, c].any() and not t[:, c].all():
            assert abs(res["c%d" % c]["roc_auc"] - metrics.roc_auc_score(t[:, c], s[:, c])) <= 1e-12
    defined = [c for c in range(6) if t[:, c].any()]
    assert len(defined) == 5
    assert abs(res["mAP"] - np.mean([metrics.average_precision_score(t[:, c], s[:, c]) for c in defined])) <= 1e-12
