"""The cross-entropy with options without a GPU: the float64 restatement of tests/ce_opts_cases.py against torch's own
cross_entropy in float64; the kernels' work simulated on the host (csrc/ce_hostsim.cpp runs csrc/ce_core.h lane by lane in the
kernels' order, in float32) against the restatement under the bounds the GPU test uses, one store per dx element, no read past
the scores; the C entries' argument errors, reported before any launch; the host-side label check and criterion parsing."""

import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ce_opts_cases as C
from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ce_hostsim") / "ce_hostsim.so")
    src = os.path.join(ROOT, PKG, "csrc", "ce_hostsim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, ci, cf = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    lib.hostsim_ce_opts.argtypes = [vp, i64, vp, i64, ci, vp, i64, cf, ci, vp, vp, vp, i64, vp, vp, vp]
    lib.hostsim_ce_workspace_bytes.argtypes = [i64]
    lib.hostsim_ce_workspace_bytes.restype = i64
    return lib


# ------------------------------------------------------------------ the restatement against torch ---------------------------

@pytest.mark.parametrize("ignore_index", [-100, 3])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("eps", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_equals_torch_in_float64(weighted, eps, reduction, ignore_index):
    x, y = C.make_case(13, 7, 40, ignore_index=ignore_index)
    w = C.make_weights(7) if weighted else None
    ref = C.restated(x, y, w, ignore_index, eps, reduction)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    loss = F.cross_entropy(x64, torch.from_numpy(y), weight=None if w is None else torch.from_numpy(w).double(),
                           ignore_index=ignore_index, label_smoothing=eps, reduction=reduction)
    loss.backward()
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-12
    assert float(np.abs(ref["dx"] - x64.grad.numpy()).max()) <= 1e-12
    ignored = y == ignore_index
    assert ignored.sum() >= 4 and not ref["dx"][ignored].any()
    assert ref["counts"] == [int(((np.argmax(x, axis=1) == y) & ~ignored).sum()), 0, int((~ignored).sum())]
    wy = np.ones(7) if w is None else w.astype(np.float64)
    assert abs(ref["den"] - wy[y[~ignored]].sum()) <= 1e-12


@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_of_an_all_ignored_batch(weighted):
    x, _ = C.make_case(6, 5, 41)
    y = np.full(6, -100, dtype=np.int64)
    w = C.make_weights(5) if weighted else None
    tw = None if w is None else torch.from_numpy(w).double()
    for reduction, want in (("mean", float("nan")), ("sum", 0.0)):
        ref = C.restated(x, y, w, -100, 0.1, reduction)
        t = float(F.cross_entropy(torch.from_numpy(x).double(), torch.from_numpy(y), weight=tw, label_smoothing=0.1, reduction=reduction))
        assert (np.isnan(ref["loss"]) and np.isnan(t)) if np.isnan(want) else (ref["loss"] == t == want)
        assert not ref["dx"].any() and ref["counts"] == [0, 0, 0] and ref["den"] == 0.0


def test_restatement_of_bad_labels_and_a_handed_in_denominator():
    x, y = C.make_case(9, 4, 42)
    ref = C.restated(x, y, None, -100, 0.0, "mean", den=12.0)
    own = C.restated(x, y, None, -100, 0.0, "mean")
    assert own["den"] == 6.0 and abs(ref["loss"] * 2 - own["loss"]) <= 1e-15 and np.allclose(ref["dx"] * 2, own["dx"], rtol=0, atol=1e-16)
    y[1], y[2] = 4, -1
    bad = C.restated(x, y, None, -100, 0.0, "mean")
    assert np.isnan(bad["loss"]) and bad["counts"][1:] == [2, 6] and not bad["dx"][[1, 2]].any()


# ------------------------------------------------------------------ the kernels on the host ----------------------------------

def run_hostsim(hostsim, x, y, w, ignore_index, eps, reduction, pad=3):
    """-> dict like the restatement's. The scores lie in a buffer of exactly rows * (K + pad) floats: the recorded highest read
    must be the last score. dx comes in NaN-filled with a pitch of K + 1; one store per element, none into the padding."""
    rows, K = x.shape
    xb = np.full((rows, K + pad), 1e30, dtype=np.float32)
    xb[:, :K] = x
    dx = np.full((rows, K + 1), np.nan, dtype=np.float32)
    writes = np.zeros((rows, K + 1), dtype=np.int32)
    loss, den = np.zeros(1, dtype=np.float32), np.zeros(1, dtype=np.float32)
    counts, max_read = np.zeros(3, dtype=np.int32), np.zeros(1, dtype=np.int64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    rc = hostsim.hostsim_ce_opts(p(xb), K + pad, p(y), rows, K, p(w), ignore_index, eps, {"mean": 0, "sum": 1}[reduction], p(den), p(loss),
                                 p(dx), K + 1, p(writes), p(counts), p(max_read))
    assert rc == 0, rc
    assert (writes[:, :K] == 1).all() and not writes[:, K:].any(), "every element of dx is written exactly once"
    return {"loss": float(loss[0]), "dx": dx[:, :K].copy(), "counts": counts.tolist(), "den": float(den[0]), "max_read": int(max_read[0])}


@pytest.mark.parametrize("rows,K", C.HOSTSIM_SHAPES)
def test_hostsim_against_the_restatement(hostsim, rows, K):
    b_loss, b_dx = C.bounds()
    x, y = C.make_case(rows, K, 50 + rows + K)
    w = C.make_weights(K)
    worst = [0.0, 0.0]
    for weighted, eps, reduction in C.OPTIONS:
        wk = w if weighted else None
        ref = C.restated(x, y, wk, -100, eps, reduction)
        got = run_hostsim(hostsim, x, y, wk, -100, eps, reduction)
        # K = 1: the gradient is exactly zero (asserted below); the float64 restatement leaves a rounding residue to divide by
        e_loss, e_dx = C.loss_err(got["loss"], ref["loss"]), C.rel(got["dx"], ref["dx"]) if K > 1 else 0.0
        worst = [max(worst[0], e_loss), max(worst[1], e_dx)]
        assert e_loss < b_loss and e_dx < b_dx, (weighted, eps, reduction, e_loss, e_dx)
        assert got["counts"] == ref["counts"]
        ignored = y == -100
        assert not got["dx"][ignored].any() and not np.signbit(got["dx"][ignored]).any()
        counted = np.flatnonzero(~ignored)
        assert got["max_read"] == counted[-1] * (K + 3) + K - 1, "no read past the last score (ignored rows are not read)"
        if reduction == "mean":
            assert got["den"] == np.float32(ref["den"])
        if K == 1:
            assert got["loss"] == 0.0 and not got["dx"].any() and float(np.abs(ref["dx"]).max()) <= 1e-15
    print("hostsim %d x %d: worst loss error %.3g (bound %.3g), worst dscores error %.3g (bound %.3g)" % (rows, K, worst[0], b_loss, worst[1], b_dx))


def test_hostsim_edge_rows(hostsim):
    """All rows ignored: NaN under the mean, 0 under the sum, dx zero, nothing read. Bad labels: NaN, counted, never an index, the
    other rows as without them. An ignore_index that is a class. The first index of a tied maximum is the prediction."""
    x, y = C.make_case(6, 65, 60)
    w = C.make_weights(65)
    gone = np.full(6, -100, dtype=np.int64)
    for reduction in ("mean", "sum"):
        got = run_hostsim(hostsim, x, gone, w, -100, 0.1, reduction)
        assert (np.isnan(got["loss"]) if reduction == "mean" else got["loss"] == 0.0) and not got["dx"].any()
        assert got["counts"] == [0, 0, 0] and got["max_read"] == -1
    clean = run_hostsim(hostsim, x, y, w, -100, 0.1, "sum")
    yb = y.copy()
    yb[1], yb[2], yb[3] = -1, 65, 2 ** 40
    got = run_hostsim(hostsim, x, yb, w, -100, 0.1, "sum")
    assert np.isnan(got["loss"]) and got["counts"][1:] == [3, clean["counts"][2]] and not got["dx"][[1, 2, 3]].any()
    keep = [0, 4, 5]
    assert np.array_equal(got["dx"][keep], clean["dx"][keep])
    y3 = np.array([3, 1, 3, 64, 0, 3], dtype=np.int64)
    got, ref = run_hostsim(hostsim, x, y3, w, 3, 0.0, "mean"), C.restated(x, y3, w, 3, 0.0, "mean")
    assert got["counts"] == ref["counts"] and got["counts"][2] == 3 and not got["dx"][[0, 2, 5]].any()
    xt = np.zeros((2, 130), dtype=np.float32)
    xt[0, [7, 64, 129]] = 2.0                       # lanes 7, 0 (second stride) and 1 (third stride): index 7 is the first
    xt[1, [129, 64]] = 2.0
    got = run_hostsim(hostsim, xt, np.array([7, 64], dtype=np.int64), None, -100, 0.0, "mean")
    assert got["counts"] == [2, 0, 2]
    got = run_hostsim(hostsim, xt, np.array([64, 129], dtype=np.int64), None, -100, 0.0, "mean")
    assert got["counts"] == [0, 0, 2]


# ------------------------------------------------------------------ the C entries ---------------------------------------------

def test_argument_errors_are_reported_before_any_launch(L, hostsim):
    lib = L.lib()
    for sym in ("mla_cross_entropy_den", "mla_cross_entropy_opts", "mla_cross_entropy_opts_workspace_bytes"):
        assert sym in L.declared_symbols() and hasattr(lib, sym)
    for rows in (1, 5, 257, 5120):
        assert lib.mla_cross_entropy_opts_workspace_bytes(rows) == hostsim.hostsim_ce_workspace_bytes(rows) >= 12 * rows
        assert lib.mla_cross_entropy_opts_workspace_bytes(rows) % 8 == 0
    fake = ctypes.c_void_p(0x1000)                       # device pointers: never dereferenced, every call below fails validation first
    E_ARG, E_SHAPE = -1, -2

    def opts(x=fake, ldx=12, labels=fake, rows=8, K=10, weight=fake, ignore=-100, eps=0.1, reduction=0, den=fake, loss=fake, dx=fake, ld_dx=10,
             counts=fake, ws=fake):
        return lib.mla_cross_entropy_opts(x, ldx, labels, rows, K, weight, ignore, eps, reduction, den, loss, dx, ld_dx, counts, ws, None)

    def den(labels=fake, rows=8, K=10, weight=fake, out=fake):
        return lib.mla_cross_entropy_den(labels, rows, K, weight, -100, out, None)

    def expect(code, rc, needle=None):
        assert rc == code, (rc, lib.mla_last_error())
        if needle:
            assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    for null in ("x", "labels", "loss", "counts", "ws"):
        expect(E_ARG, opts(**{null: None}), "null")
    for rows in (0, -3):
        expect(E_ARG, opts(rows=rows), "rows")
        expect(E_ARG, den(rows=rows), "rows")
    for K in (0, -1, 1025):
        expect(E_SHAPE, opts(K=K, ldx=2048, ld_dx=2048), "classes")
        expect(E_SHAPE, den(K=K), "classes")
    expect(E_ARG, opts(ldx=9), "pitch")
    expect(E_ARG, opts(ld_dx=9), "pitch")
    for eps in (-0.01, 1.5, float("nan")):
        expect(E_ARG, opts(eps=eps), "label_smoothing")
    for code in (-1, 2, 7):
        expect(E_ARG, opts(reduction=code), "reduction")
    expect(E_ARG, opts(den=None), "den")
    expect(E_ARG, opts(ws=ctypes.c_void_p(0x1004)), "aligned")
    expect(E_ARG, den(labels=None), "null")
    expect(E_ARG, den(out=None), "null")


# ------------------------------------------------------------------ host logic -------------------------------------------------

def test_check_labels_ignoring_lets_the_ignored_label_through():
    ops = importlib.import_module(PKG + ".ops")
    y = torch.tensor([0, 9, -100, 3, -100])
    ops.check_labels_ignoring(y, 10, -100)
    ops.check_labels_ignoring(torch.tensor([3, 3, 0, 9]), 10, 3)            # an ignored class that lies inside the range
    ops.check_labels_ignoring(torch.tensor([12, 0, 9, 12]), 10, 12)         # and one outside
    ops.check_labels_ignoring(torch.tensor([-100, -100]), 10, -100)         # nothing left to check
    ops.check_labels_ignoring(torch.zeros(0, dtype=torch.int64), 10, -100)
    for bad in (-1, 10):
        with pytest.raises(IndexError, match=str(bad)):
            ops.check_labels_ignoring(torch.tensor([0, bad, -100]), 10, -100)
    with pytest.raises(IndexError):
        ops.check_labels_ignoring(torch.tensor([0, -100]), 10, 3)           # -100 is not the ignored label here
    with pytest.raises(IndexError):
        ops.check_labels(y, 10)                                             # the plain check still refuses it


def test_criterion_parsing_refuses_what_the_step_cannot_do():
    TR = importlib.import_module(PKG + ".train")
    CE = torch.nn.CrossEntropyLoss
    got = TR.parse_criterion(CE(), 10)
    assert got == {"weight": None, "ignore_index": -100, "label_smoothing": 0.0, "reduction": "mean"}
    w = torch.linspace(0.5, 2.0, 10, dtype=torch.float64)
    got = TR.parse_criterion(CE(weight=w, ignore_index=3, label_smoothing=0.1, reduction="sum"), 10)
    assert got["weight"].dtype == torch.float32 and torch.equal(got["weight"], w.float()) and not got["weight"].is_cuda
    assert (got["ignore_index"], got["label_smoothing"], got["reduction"]) == (3, 0.1, "sum")
    assert TR.parse_criterion(CE(weight=torch.tensor([0.0, 1.0])), 2)["weight"].tolist() == [0.0, 1.0]      # one zero weight is fine
    with pytest.raises(ValueError, match="scalar"):
        TR.parse_criterion(CE(reduction="none"), 10)
    for bad in (torch.ones(9), torch.ones(11), torch.ones(2, 5)):
        with pytest.raises(ValueError, match="classes"):
            TR.parse_criterion(CE(weight=bad), 10)
    neg, nan, inf = torch.ones(10), torch.ones(10), torch.ones(10)
    neg[4], nan[4], inf[4] = -0.5, float("nan"), float("inf")
    for bad in (neg, nan, inf):
        with pytest.raises(ValueError, match="finite and non-negative"):
            TR.parse_criterion(CE(weight=bad), 10)
    with pytest.raises(ValueError, match="all zero"):
        TR.parse_criterion(CE(weight=torch.zeros(10)), 10)
    with pytest.raises(ValueError, match="float"):
        TR.parse_criterion(CE(weight=torch.ones(10, dtype=torch.int64)), 10)
    for eps in (1.5, -0.1):
        crit = CE()
        crit.label_smoothing = eps
        with pytest.raises(ValueError, match="label_smoothing"):
            TR.parse_criterion(crit, 10)
    with pytest.raises(TypeError):
        TR.parse_criterion(torch.nn.BCEWithLogitsLoss(), 10)
    with pytest.raises(NotImplementedError):
        TR.parse_criterion(CE(), 1025)
