"""GPU tests of the f32 training kernels of the head and of the optimiser step (csrc/mla_head.hip backward parts,
csrc/train_kernels.hip), ONE KERNEL AT A TIME against a float64 torch/numpy computation on the CPU from the same f32 input
values. The composed tests (golden loss curves, head gradients against the oracle's autograd) reach these kernels at one shape with
dense tensors; here every branch of each kernel is entered on its own: dead lanes of the 16-lane attention groups, the
grid-stride loops behind capped grids, the vector / scalar switch of the BatchNorm backward sums, strided operands, accumulate /
want_dx / batch_stats, SyncBN's global-vs-local sums, both grid choices of linear_small_bwd, label errors and arg-max ties of the
cross entropy, edge tiles of the transpose.

Two kinds of bounds:
  derived   kernels without transcendental functions: an f32 chain of P roundings is within P * 2^-24 * sum|terms| of float64;
            the bound is computed per output element from the float64 reference, P is counted in the test that uses it.
  measured  kernels with __expf / __logf / the fast sigmoid / Adam's division chain: worst relative error (max|got - ref| /
            max|ref| per tensor) over the whole parametrization as measured on the MI355X, times 4, never looser than the composed
            head test (1e-4 on outputs, 2e-3 on gradients): the table MEASURED below.
"""

import importlib
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # unit roundoff of float32
EPS = 1e-5                # ops.BN_EPS


def _grid_cap():
    """Threads of the largest grid that train_kernels.hip grid_for() (adam_step, axpy) and the bn_apply / bn_bwd_apply launchers of
    mla_head.hip start, READ FROM THE SOURCES: all three say `(n + 255) / 256 < CAP ? ... : CAP` with 256-thread blocks. If a cap
    changes, the sizes below follow; if the launchers are rewritten, this fails instead of leaving the grid-stride loops untested."""
    csrc = os.path.join(ROOT, PKG, "csrc")
    with open(os.path.join(csrc, "train_kernels.hip")) as f:
        caps = re.findall(r"unsigned grid_for\(int64_t n\) \{ return unsigned\(\(n \+ 255\) / 256 < (\d+) \? \(n \+ 255\) / 256 : (\d+)\); \}", f.read())
    assert len(caps) == 1, "grid_for() of train_kernels.hip is not in the form this test reads"
    with open(os.path.join(csrc, "mla_head.hip")) as f:
        head = re.findall(r"unsigned\(\(total \+ 255\) / 256 < (\d+) \? \(total \+ 255\) / 256 : (\d+)\)", f.read())
    assert len(head) == 2, "the bn_apply / bn_bwd_apply launchers of mla_head.hip are not in the form this test reads"
    blocks = {int(v) for pair in caps + head for v in pair}
    assert len(blocks) == 1, blocks
    return blocks.pop() * 256


GRID_CAP = _grid_cap()    # 8192 blocks of 256 threads as the sources stand

# Bounds of the kernels whose error is not derivable from the code: name -> (worst relative error measured on the MI355X over the
# test's whole parametrization, bound). The rule is bound = 4 x the measured value, capped by what the composed head test grants
# (1e-4 on outputs, 2e-3 on gradients); every bound here is far below its cap. The worst attention figures come from the spread-60
# case (10, 16, 33), the worst cross-entropy gradient from the +-80 logits. "adam v" is not noise: beta2 = 0.999 rounds to
# 0.99900001 in f32, so the kernel's 1.f - b2 is 1.29e-5 below 0.001, and the second moment with it.
MEASURED = {
    "attention y": (3.34e-7, 4 * 3.34e-7), "attention att": (6.67e-7, 4 * 6.67e-7), "attention cla": (1.08e-7, 4 * 1.08e-7),
    "attention du_v": (2.76e-6, 4 * 2.76e-6), "attention du_f": (5.91e-7, 4 * 5.91e-7),
    "bn_apply sigmoid": (1.10e-7, 4 * 1.10e-7),
    "cross_entropy loss": (7.23e-8, 4 * 7.23e-8), "cross_entropy dscores": (3.74e-6, 4 * 3.74e-6),
    "adam update": (2.00e-6, 4 * 2.00e-6), "adam m": (3.09e-7, 4 * 3.09e-7), "adam v": (1.30e-5, 4 * 1.30e-5),
}
assert all(b <= (2e-3 if ("du_" in k or "dscores" in k) else 1e-4) for k, (_, b) in MEASURED.items())


def measured(name, err):
    """Print the figure, then assert it against the table."""
    print("%s: %.3g (recorded %s, bound %.3g)" % (name, err, MEASURED[name][0], MEASURED[name][1]))
    assert err < MEASURED[name][1], (name, err)


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


def rnd(W, seed, stream, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(W.uniform(seed, stream, int(np.prod(shape)), lo=lo, hi=hi)).reshape(shape)


def rel(got, ref):
    """max|got - ref| / max|ref| (0 when both are all-zero)."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    d, m = float((got - ref).abs().max()), float(ref.abs().max())
    return d / m if m > 0 else d


def within(got, ref, bound, what):
    """Per-element derived bound; prints the worst ratio error / bound before asserting."""
    got, ref = got.double().cpu(), ref.double()
    ratio = float(((got - ref).abs() / (bound + 1e-300)).max())
    print("%s: worst |error| / bound = %.3g" % (what, ratio))
    assert ratio <= 1.0, (what, ratio)


def strided(t, left=1, right=2, fill=0.0):
    """The same values as a column slice of a wider CUDA tensor: pitch = cols + left + right, start misaligned by 4 * left bytes."""
    buf = torch.full((t.shape[0], t.shape[1] + left + right), fill, dtype=t.dtype, device="cuda")
    view = buf[:, left:left + t.shape[1]]
    view.copy_(t)
    return view


# ----------------------------------------------------------------------------------------- attention pooling ----

ATT_CASES = [  # T, K, bags, spread of the pre-softmax values
    (16, 16, 33, 5.0), (1, 1, 1, 5.0), (7, 10, 15, 5.0), (10, 10, 17, 5.0), (10, 16, 33, 60.0), (16, 1, 17, 5.0), (1, 16, 15, 5.0),
    (7, 1, 1, 5.0), (10, 10, 1, 60.0)]


def _attention_reference(z, nv, nf, T):
    """float64: u = BatchNorm1d(T) with the given statistics (channel = time slot), att = softmax_k(u_v), cla = sigmoid(u_f),
    y = sum_t cla att / sum_t att. Returns leaves u_v, u_f (for autograd) and y."""
    def bn(p):
        m, v, g, b = (q.double().reshape(1, T, 1) for q in p)
        return ((z.double() - m) / torch.sqrt(v + EPS) * g + b).detach().requires_grad_(True)
    u_v, u_f = bn(nv), bn(nf)
    att, cla = torch.softmax(u_v, dim=2), torch.sigmoid(u_f)
    y = (cla * att).sum(dim=1) / att.sum(dim=1)
    return u_v, u_f, att, cla, y


@pytest.mark.parametrize("T,K,bags,spread", ATT_CASES)
def test_attention_pool_and_its_backward_match_float64(ops, W, T, K, bags, spread):
    """mla_attention_pool / mla_attention_pool_bwd: 16 lanes per bag (T < 16 leaves dead lanes, bags % 16 != 0 dead groups), K <= 16
    classes in registers. y goes into a column slice of a wider tensor (ldy > K; the rest keeps its sentinel), save=True and
    save=False must give the same bits, spread 60 exercises the max subtraction of the softmax (exp(60) overflows nothing only
    because of it). Backward: from the SAVED att / cla and a strided dy, against float64 autograd w.r.t. the two BatchNorm outputs.
    Bounds: MEASURED["attention ..."]."""
    seed = 300 + T * 17 + K
    z = rnd(W, seed, 1, (bags, T, K), -2.0, 2.0)        # |normalised z| <= 2.6 / sqrt(4 / 6) = 3.2
    nv = (rnd(W, seed, 2, (T,), -0.6, 0.6), rnd(W, seed, 3, (T,), 0.5, 2.0) * 4 / 3, rnd(W, seed, 4, (T,), 0.5, 1.5) * spread / 4.8,
          rnd(W, seed, 5, (T,), -0.5, 0.5))
    nf = (rnd(W, seed, 6, (T,), -0.6, 0.6), rnd(W, seed, 7, (T,), 0.5, 2.0) * 4 / 3, rnd(W, seed, 8, (T,), 0.5, 1.5),
          rnd(W, seed, 9, (T,), -0.5, 0.5))
    u_v, u_f, att64, cla64, y64 = _attention_reference(z, nv, nf, T)
    # the inputs, not the kernel: |u_v| <= 2.6 * 1.23 * 1.5 * spread / 4.8 + 0.5 always; a single time slot may draw a small gamma,
    # so only the spread-60 cases (ten slots) are required to reach the range that needs the max subtraction
    top = float(u_v.detach().abs().max())
    assert top <= spread + 0.5 and (spread < 60.0 or top > 0.5 * spread), top
    zc = z.reshape(bags * T, K).cuda()
    nvc, nfc = [p.cuda() for p in nv], [p.cuda() for p in nf]
    sentinel = -7.25
    ybuf = torch.full((bags, K + 5), sentinel, device="cuda")
    att, cla = ops.attention_pool(zc, bags, T, K, nvc, nfc, ybuf[:, 2:2 + K], save=True)
    ybuf2 = torch.full((bags, K + 5), sentinel, device="cuda")
    assert ops.attention_pool(zc, bags, T, K, nvc, nfc, ybuf2[:, 2:2 + K], save=False) == (None, None)
    assert torch.equal(ybuf, ybuf2), "y must not depend on whether att / cla are saved"
    assert bool((ybuf[:, :2] == sentinel).all()) and bool((ybuf[:, 2 + K:] == sentinel).all()), "columns outside the slice were written"
    measured("attention y", rel(ybuf[:, 2:2 + K], y64))
    measured("attention att", rel(att.reshape(bags, T, K), att64))
    measured("attention cla", rel(cla.reshape(bags, T, K), cla64))

    dy = rnd(W, seed, 10, (bags, K))
    y64.backward(dy.double())
    du_v, du_f = ops.attention_pool_bwd(strided(dy), att, cla, bags, T, K)
    if T == 1:
        # one time slot: y = cla, so d y / d u_v is identically zero. Float64 autograd returns its own rounding noise (1e-17) and the
        # kernel an exact 0 (att / att = 1, cla - y = 0); noise is no scale to divide by, so the error is taken relative to the terms
        # that cancel, dy * att / sum_t att = dy
        assert float(u_v.grad.abs().max()) < 1e-14
        measured("attention du_v", float((du_v.reshape(bags, T, K).double().cpu() - u_v.grad).abs().max()) / float(dy.abs().max()))
    else:
        measured("attention du_v", rel(du_v.reshape(bags, T, K), u_v.grad))
    measured("attention du_f", rel(du_f.reshape(bags, T, K), u_f.grad))


# ------------------------------------------------------------------------------------------------ BatchNorm ----

def _bn_channels(t, mode, period):
    """View with the channel on axis 1 and everything reduced on axes 0 and 2."""
    rows, cols = t.shape
    return t.reshape(rows // period, period, cols) if mode == 0 else t.reshape(rows, cols, 1)


def bn_reference(x, dy, gamma, beta, mode, period, act, keep, drop_scale, stats=None):
    """float64 autograd through y = act((x - mean) rsqrt(var + eps) gamma + beta) [* keep * drop_scale] with the batch statistics
    computed here (stats=None) or FIXED statistics (mean, var). Returns the forward output, the three gradients and the derived
    per-element bounds.

    Rounding count of the kernels (u = 2^-24), on top of exact float64 sums:
      xhat = (x - mean) * inv: mean and var arrive rounded to f32 (2), var + eps, sqrtf, 1/ (3), the subtraction and the product (2)
             -> 7 roundings, each at most u * (|x| + |mean|) * inv in xhat's units [the subtraction may cancel: the bound uses
             |x| + |mean|, not |x - mean|]
      g    = gradient through the activation: exact for none, 1 for ReLU (dy * drop_scale), 4 for the sigmoid (yout arrives rounded,
             1 - y, two products), each at most u * |dy| * s with s = 1 / drop_scale / yout
      dbeta  = f32(sum g):           (rounding of g + 1) * u * sum|g|
      dgamma = f32(sum g xhat):      (g + 7 + 1) * u * sum |g| (|x| + |mean|) inv
      dx     = gamma inv (g - sg - xhat sgx): sg, sgx are those sums / count rounded to f32 (their own roundings as above + 2);
               then xhat sgx, two subtractions, gamma * inv, the last product (5 + 3 for inv) -> with A = mean|g| and
               B = mean |g| (|x| + |mean|) inv per channel, every term is bounded by
               T = |gamma| inv (|g| + A + (|x| + |mean|) inv B). Roundings on the worst term xhat sgx: 7 (xhat) + 12 (sgx =
               4 for g + 7 for xhat + 1) + 1 (product) = 20, + 2 subtractions + 5 (inv 3, gamma inv, last product) = 27 to first
               order; P = 28.
    """
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    xc = _bn_channels(x64, mode, period)
    if stats is None:
        mean, var = xc.mean(dim=(0, 2), keepdim=True), xc.var(dim=(0, 2), unbiased=False, keepdim=True)
    else:
        mean, var = (s.double().reshape(1, -1, 1) for s in stats)
    inv = torch.rsqrt(var + EPS)
    v = (xc - mean) * inv * g64.reshape(1, -1, 1) + b64.reshape(1, -1, 1)
    if act == 1:
        v = torch.relu(v)
    elif act == 2:
        v = torch.sigmoid(v)
    v = v.reshape(x.shape)
    if keep is not None:
        v = v * keep.reshape(x.shape).double() * drop_scale
    v.backward(dy.double())
    with torch.no_grad():
        y = v.detach()
        if act == 1:
            gabs = torch.where(y > 0, dy.double().abs() * drop_scale, torch.zeros_like(y))
        elif act == 2:
            gabs = dy.double().abs() * y
        else:
            gabs = dy.double().abs()
        n_g = {0: 0, 1: 1, 2: 4}[act]
        span = (_bn_channels(x.double().abs(), mode, period) + mean.abs()) * inv              # (|x| + |mean|) inv
        gc = _bn_channels(gabs, mode, period)
        A, B = gc.mean(dim=(0, 2), keepdim=True), (gc * span).mean(dim=(0, 2), keepdim=True)
        cnt = gc.shape[0] * gc.shape[2]
        T = g64.detach().abs().reshape(1, -1, 1) * inv * (gc + A + span * B)
        bounds = {"dx": (28 * U * T).reshape(x.shape), "dbeta": ((n_g + 1) * U * A * cnt).reshape(-1),
                  "dgamma": ((n_g + 8) * U * B * cnt).reshape(-1)}
    return {"y": y, "dx": x64.grad, "dgamma": g64.grad, "dbeta": b64.grad, "mean": mean.detach().reshape(-1).float(),
            "var": var.detach().reshape(-1).float(), "bounds": bounds, "gabs": gabs}


def _bn_inputs(W, seed, rows, cols, ch, act):
    x = rnd(W, seed, 1, (rows, cols), -1.0, 3.0)
    dy = rnd(W, seed, 2, (rows, cols))
    gamma, beta = rnd(W, seed, 3, (ch,), 0.5, 1.5), rnd(W, seed, 4, (ch,), -0.5, 0.5)
    keep = torch.from_numpy(W.keep_mask(seed, 5, rows * cols, 0.5)) if act == 1 else None
    return x, dy, gamma, beta, keep, (2.0 if act == 1 else 1.0)


def _run_bn_backward(ops, ref, x, dy, gamma, act, drop_scale, mode, period, layout, what, **kw):
    """bn_backward on the reference's own forward output and statistics (rounded to f32), in a dense or strided layout."""
    put = (lambda t: t.cuda()) if layout == "dense" else strided
    ch = gamma.numel()
    dgamma, dbeta = torch.full((ch,), 9.0, device="cuda"), torch.full((ch,), 9.0, device="cuda")
    yout = put(ref["y"].float()) if act else None
    dx = ops.bn_backward(put(x), put(dy), yout, act, drop_scale, mode, period, ref["mean"].cuda(), ref["var"].cuda(), gamma.cuda(),
                         ops._local(), dgamma, dbeta, **kw)
    within(dgamma, ref["dgamma"], ref["bounds"]["dgamma"], what + " dgamma")
    within(dbeta, ref["dbeta"], ref["bounds"]["dbeta"], what + " dbeta")
    return dx


BN_CASES = [  # mode, period, rows, cols, act
    (0, 1, 5, 10, 0), (0, 10, 60, 600, 1), (0, 10, 60, 601, 0), (0, 10, 60, 600, 2), (0, 64, 192, 10, 0), (0, 10, 6000, 10, 1),
    (0, 1, 1000, 600, 0), (0, 64, 64 * 520, 10, 2),
    (1, 0, 5, 1, 0), (1, 0, 5, 10, 1), (1, 0, 5, 64, 2), (1, 0, 1000, 1, 2), (1, 0, 1000, 10, 0), (1, 0, 1000, 64, 1)]


@pytest.mark.parametrize("mode,period,rows,cols,act", BN_CASES)
def test_bn_backward_matches_float64_autograd_in_both_layouts(ops, W, mode, period, rows, cols, act):
    """mla_bn_bwd_sums + mla_bn_bwd_apply. mode 0 (channel = row % period): periods 1 / 10 / 64, rows / period below and above the
    512 partial-producing blocks (a block then owns several periods of rows); mode 1 (channel = column): 256 threads are not a
    multiple of 10 columns. Every case runs dense (16-byte loads where cols % 4 == 0) AND as x[:, 1:]-style views of wider tensors
    (misaligned by 4 bytes, pitch not a multiple of 4: the scalar path); 601 columns are scalar in both. The forward output handed
    to the kernel is the reference's own, rounded to f32, so the ReLU mask is the reference's mask; bounds derived in bn_reference."""
    ch = period if mode == 0 else cols
    x, dy, gamma, beta, keep, drop_scale = _bn_inputs(W, 400 + rows + cols, rows, cols, ch, act)
    ref = bn_reference(x, dy, gamma, beta, mode, period, act, keep, drop_scale)
    for layout in ("dense", "strided"):
        what = "bn_backward mode %d period %d %dx%d act %d %s" % (mode, period, rows, cols, act, layout)
        dx = _run_bn_backward(ops, ref, x, dy, gamma, act, drop_scale, mode, period, layout, what)
        within(dx, ref["dx"], ref["bounds"]["dx"], what + " dx")


def test_bn_backward_options_accumulate_no_dx_and_fixed_statistics(ops, W):
    """accumulate=True adds to a pre-filled dx (one more rounding on |pre| + |v|); want_dx=False still writes dgamma / dbeta and
    touches no dx; batch_stats=False (eval-mode forward, fixed running statistics): dx = gamma rstd g, the sums still feed
    dgamma / dbeta."""
    mode, period, rows, cols, act = 0, 10, 70, 600, 1
    x, dy, gamma, beta, keep, drop_scale = _bn_inputs(W, 431, rows, cols, period, act)
    ref = bn_reference(x, dy, gamma, beta, mode, period, act, keep, drop_scale)
    pre = rnd(W, 431, 6, (rows, cols), -2.0, 2.0)
    dx = pre.cuda()
    out = _run_bn_backward(ops, ref, x, dy, gamma, act, drop_scale, mode, period, "dense", "bn_backward accumulate", dx=dx, accumulate=True)
    assert out is dx
    total = pre.double() + ref["dx"]
    within(dx, total, ref["bounds"]["dx"] + U * (pre.double().abs() + ref["dx"].abs()), "bn_backward accumulate dx")
    assert _run_bn_backward(ops, ref, x, dy, gamma, act, drop_scale, mode, period, "dense", "bn_backward want_dx=False", want_dx=False) is None
    # fixed statistics
    stats = (rnd(W, 431, 7, (period,), 0.5, 1.5), rnd(W, 431, 8, (period,), 0.5, 2.0))
    fixed = bn_reference(x, dy, gamma, beta, mode, period, act, keep, drop_scale, stats=stats)
    inv = torch.rsqrt(stats[1].double() + EPS).reshape(1, -1, 1)
    g = torch.where(fixed["y"] > 0, dy.double() * drop_scale, torch.zeros_like(fixed["y"]))
    expect = (gamma.double().reshape(1, -1, 1) * inv * _bn_channels(g, mode, period)).reshape(rows, cols)
    assert float((expect - fixed["dx"]).abs().max()) < 1e-12                  # autograd with fixed statistics IS gamma rstd g
    dx = _run_bn_backward(ops, fixed, x, dy, gamma, act, drop_scale, mode, period, "dense", "bn_backward batch_stats=False", batch_stats=False)
    within(dx, expect, fixed["bounds"]["dx"], "bn_backward batch_stats=False dx")


def test_bn_apply_and_bn_backward_beyond_the_grid_cap(ops, W):
    """400 bags x 10 x 600 = 2 400 000 elements > 8192 blocks x 256 threads: the grid-stride loops of bn_apply_kernel and
    bn_bwd_apply_kernel take a second trip. Forward (ReLU + keep-mask, derived: v = (x - mean) inv gamma + beta is 7 roundings for
    xhat + 3, every term below (|x| + |mean|) inv |gamma| + |beta|, times drop_scale 2 exactly) and backward on the same data."""
    mode, period, rows, cols, act = 0, 10, 4000, 600, 1
    assert rows * cols > GRID_CAP
    x, dy, gamma, beta, keep, drop_scale = _bn_inputs(W, 433, rows, cols, period, act)
    ref = bn_reference(x, dy, gamma, beta, mode, period, act, keep, drop_scale)
    y = ops.bn_apply(x.cuda(), mode, period, ref["mean"].cuda(), ref["var"].cuda(), gamma.cuda(), beta.cuda(), act=act,
                     keep_mask=keep.cuda(), drop_scale=drop_scale)
    m = ref["mean"].double().reshape(1, -1, 1)
    inv = torch.rsqrt(ref["var"].double() + EPS).reshape(1, -1, 1)
    T = ((_bn_channels(x.double().abs(), mode, period) + m.abs()) * inv * gamma.double().abs().reshape(1, -1, 1)
         + beta.double().abs().reshape(1, -1, 1)).reshape(rows, cols) * drop_scale
    within(y, ref["y"], 10 * U * T, "bn_apply 4000x600 relu + mask")
    assert bool((y.cpu()[keep.reshape(rows, cols) == 0] == 0).all())
    dx = _run_bn_backward(ops, ref, x, dy, gamma, act, drop_scale, mode, period, "dense", "bn_backward 4000x600")
    within(dx, ref["dx"], ref["bounds"]["dx"], "bn_backward 4000x600 dx")


@pytest.mark.parametrize("mode,period,rows,cols", [(0, 10, 70, 600), (0, 10, 70, 601), (1, 0, 1000, 10), (1, 0, 37, 64)])
def test_bn_apply_sigmoid_and_plain_match_float64(ops, W, mode, period, rows, cols):
    """bn_apply with the fast sigmoid (1 / (1 + __expf(-v))) into a strided output, and without activation under the derived bound.
    Bound: MEASURED["bn_apply sigmoid"]."""
    ch = period if mode == 0 else cols
    x, dy, gamma, beta, _, _ = _bn_inputs(W, 440 + cols, rows, cols, ch, 0)
    ref0 = bn_reference(x, dy, gamma, beta, mode, period, 0, None, 1.0)
    ref2 = bn_reference(x, dy, gamma, beta, mode, period, 2, None, 1.0)
    args = (mode, period, ref0["mean"].cuda(), ref0["var"].cuda(), gamma.cuda(), beta.cuda())
    m, inv = ref0["mean"].double().reshape(1, -1, 1), torch.rsqrt(ref0["var"].double() + EPS).reshape(1, -1, 1)
    T = ((_bn_channels(x.double().abs(), mode, period) + m.abs()) * inv * gamma.double().abs().reshape(1, -1, 1)
         + beta.double().abs().reshape(1, -1, 1)).reshape(rows, cols)
    out = torch.full((rows, cols + 6), 5.5, device="cuda")                 # a pitch of its own: not x's
    ops.bn_apply(strided(x), *args, act=0, out=out[:, 1:1 + cols])
    within(out[:, 1:1 + cols], ref0["y"], 10 * U * T, "bn_apply plain %dx%d" % (rows, cols))
    assert bool((out[:, :1] == 5.5).all()) and bool((out[:, 1 + cols:] == 5.5).all())
    y2 = ops.bn_apply(x.cuda(), *args, act=2)
    measured("bn_apply sigmoid", rel(y2, ref2["y"]))


class _TwoShards:
    """What bn_backward needs of ops.Dist for a two-rank SyncBN group, on one GPU: the all-reduce adds the OTHER shard's sums."""
    bn_active, bn_world = True, 2

    def __init__(self, other=None):
        self.other, self.recorded = other, None

    def all_reduce_sum(self, t, tag="other"):
        assert tag == "syncbn_bwd"
        self.recorded = t.clone()
        if self.other is not None:
            t += self.other
        return t


@pytest.mark.parametrize("act", [0, 1])
def test_syncbn_backward_algebra_on_two_unequal_shards(ops, W, act):
    """sums_global != sums_local in bn_bwd_apply: a batch of 19 bags split 7 + 12. Each shard runs bn_backward with the GLOBAL
    float64 statistics; a first pass records each shard's local sums, the second pass's all-reduce adds the other shard's. dx of the
    shards, concatenated, must be the single-batch dx (global sums drive dx), and dgamma / dbeta of the shards must ADD UP to the
    single-batch ones (local sums drive them; the gradient all-reduce adds the ranks). Shards of different sizes pass the global
    count (the training step's contract is equal shards: count = local count x world)."""
    mode, period, cols, bags, cut = 0, 10, 600, 19, 7
    rows = bags * period
    x, dy, gamma, beta, keep, drop_scale = _bn_inputs(W, 450 + act, rows, cols, period, act)
    ref = bn_reference(x, dy, gamma, beta, mode, period, act, keep, drop_scale)
    mean, var, gam = ref["mean"].cuda(), ref["var"].cuda(), gamma.cuda()
    yout = ref["y"].float() if act else None
    parts = [slice(0, cut * period), slice(cut * period, rows)]

    def shard(sl, dist):
        dg, db = torch.empty(period, device="cuda"), torch.empty(period, device="cuda")
        dx = ops.bn_backward(x[sl].cuda(), dy[sl].cuda(), yout[sl].cuda() if act else None, act, drop_scale, mode, period, mean, var, gam,
                             dist, dg, db, count=bags * cols)
        return dx, dg, db

    recorders = [_TwoShards(), _TwoShards()]
    for sl, d in zip(parts, recorders):
        shard(sl, d)
    assert not torch.equal(recorders[0].recorded, recorders[1].recorded)
    outs = [shard(parts[0], _TwoShards(recorders[1].recorded)), shard(parts[1], _TwoShards(recorders[0].recorded))]
    within(torch.cat([outs[0][0], outs[1][0]]), ref["dx"], ref["bounds"]["dx"], "syncbn two shards dx")
    within(outs[0][1].double() + outs[1][1].double(), ref["dgamma"], ref["bounds"]["dgamma"] + U * ref["dgamma"].abs(), "syncbn dgamma sum")
    within(outs[0][2].double() + outs[1][2].double(), ref["dbeta"], ref["bounds"]["dbeta"] + U * ref["dbeta"].abs(), "syncbn dbeta sum")
    # and against the single-batch run of the same kernels: both are within the bound of float64, so within two bounds of each other
    dg1, db1 = torch.empty(period, device="cuda"), torch.empty(period, device="cuda")
    dx1 = ops.bn_backward(x.cuda(), dy.cuda(), yout.cuda() if act else None, act, drop_scale, mode, period, mean, var, gam, ops._local(), dg1, db1)
    within(torch.cat([outs[0][0], outs[1][0]]), dx1.double().cpu(), 2 * ref["bounds"]["dx"], "syncbn two shards vs one batch")
    # a shard on its own sums is a different (per-shard BatchNorm) gradient: the test can tell the two apart
    alone = shard(parts[0], ops._local())[0]
    assert float((alone.double().cpu() - ref["dx"][parts[0]]).abs().max()) > 100 * float(ref["bounds"]["dx"].max())


# ------------------------------------------------------------------------------------------- linear_small_bwd ----

@pytest.mark.parametrize("M,N,K", [(1, 10, 600), (37, 10, 600), (5120, 10, 600), (70, 3, 5), (300, 16, 4)])
def test_linear_small_bwd_matches_float64(ops, W, M, N, K):
    """da = dz W (N-term fma chain per element: N roundings), dW = dz^T a and db = sum dz (double accumulation, one rounding to
    f32; 2 allowed). The grid is max(blocks for da, blocks for dW + db): (1, 10, 600) and (37, ...) are dW-dominant with M below one
    wave, (5120, ...) and (300, 16, 4) da-dominant. a and dz are row-strided views."""
    a, w, dz = rnd(W, 500 + M, 1, (M, K)), rnd(W, 500 + M, 2, (N, K)), rnd(W, 500 + M, 3, (M, N))
    dw, db = torch.full((N, K), 9.0, device="cuda"), torch.full((N,), 9.0, device="cuda")
    da = ops.linear_small_bwd(strided(a), w.cuda(), strided(dz, 3, 1), dw, db)
    a64, w64, z64 = a.double(), w.double(), dz.double()
    within(da, z64 @ w64, N * U * (z64.abs() @ w64.abs()), "linear_small_bwd %dx%dx%d da" % (M, N, K))
    within(dw, z64.t() @ a64, 2 * U * (z64.abs().t() @ a64.abs()), "linear_small_bwd dW")
    within(db, z64.sum(dim=0), 2 * U * z64.abs().sum(dim=0), "linear_small_bwd db")


# ---------------------------------------------------------------------------------------------- cross entropy ----

def _ce_inputs(W, rows, K, spread, seed):
    x = rnd(W, seed, 1, (rows, K), -spread, spread)
    if K >= 2:                                          # exact ties of the maximum: the first index wins (torch.argmax)
        for r in range(0, rows, 5):
            i, j = (r // 5) % K, (r // 5 + 1 + (r // 35) % (K - 1)) % K
            x[r, i] = x[r, j] = float(x[r].max()) + 0.25
    labels = torch.from_numpy(W.bits24(seed, 2, rows) % K)
    if K >= 2:
        for r in range(0, rows, 10):                    # half of the tied rows: the label IS one of the tied indices
            labels[r] = int(torch.argmax(x[r]))
    return x, labels


@pytest.mark.parametrize("K", [1, 2, 10])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 5120])
def test_cross_entropy_matches_float64(ops, W, rows, K):
    """mla_cross_entropy: one block of 256 threads strides over the rows (fewer, exactly 256, one more, 20 per thread). Scores
    are a column slice of a wider tensor; inv_total is the GLOBAL batch's (not 1 / rows). Ties of the maximum: the first index counts
    as the prediction. Logits spread over +-80 for 257 rows (lse = max + log(sum exp(x - max)) needs the max subtraction).
    Bounds: MEASURED["cross_entropy ..."]; the loss error is relative to max(|loss|, 1)."""
    spread = 80.0 if rows == 257 else 4.0
    x, labels = _ce_inputs(W, rows, K, spread, 600 + rows + K)
    inv_total = 1.0 / (rows + 3)
    x64 = x.double().requires_grad_(True)
    ref = F.cross_entropy(x64, labels, reduction="sum") * inv_total
    ref.backward()
    ref = ref.detach()
    hits_ref = int((torch.argmax(x, dim=1) == labels).sum())
    loss, d, hits = ops.cross_entropy(strided(x, 2, 1), labels.cuda(), inv_total)
    assert d.is_contiguous() and tuple(d.shape) == (rows, K)
    assert hits.tolist() == [hits_ref, 0] and ops.raise_on_bad_labels(hits) == hits_ref
    measured("cross_entropy loss", abs(float(loss) - float(ref)) / max(abs(float(ref)), 1.0))
    measured("cross_entropy dscores", rel(d, x64.grad))
    if K == 1:
        assert float(loss) == 0.0 and not bool(d.any())
    loss2, d2, hits2 = ops.cross_entropy(strided(x, 2, 1), labels.cuda(), inv_total, want_grad=False)
    assert d2 is None and torch.equal(loss2, loss) and torch.equal(hits2, hits)


@pytest.mark.parametrize("rows,K", [(257, 10), (5, 2)])
def test_cross_entropy_refuses_labels_outside_the_classes(ops, W, rows, K):
    """Device labels outside [0, K) are never used as an index: NaN loss, hits[1] = their number, their dscores rows zero, every
    other row as without them; raise_on_bad_labels turns the counter into the reference's exception."""
    x, labels = _ce_inputs(W, rows, K, 4.0, 650 + rows)
    bad = {0: -1, rows // 2: K, rows - 1: -100, 3: 2 ** 40}
    good = labels.clone()
    for r, v in bad.items():
        labels[r] = v
    inv_total = 1.0 / rows
    _, d_good, hits_good = ops.cross_entropy(x.cuda(), good.cuda(), inv_total)
    loss, d, hits = ops.cross_entropy(x.cuda(), labels.cuda(), inv_total)
    assert bool(torch.isnan(loss).all()) and int(hits[1]) == len(bad)
    keep = torch.ones(rows, dtype=torch.bool)
    keep[list(bad)] = False
    assert not bool(d.cpu()[~keep].any()) and torch.equal(d.cpu()[keep], d_good.cpu()[keep])
    assert int(hits[0]) == int((torch.argmax(x, dim=1)[keep] == good[keep]).sum())
    with pytest.raises(IndexError):
        ops.raise_on_bad_labels(hits)
    with pytest.raises(IndexError):
        ops.check_labels(labels, K)                     # the host-side check of the same condition


# ------------------------------------------------------------------------------------------- Adam, axpy, transpose ----

SIZES = [1, 255, 257, GRID_CAP + 257]


@pytest.mark.parametrize("n", SIZES)
def test_adam_step_matches_torch_adam_in_float64(ops, W, n):
    """Five steps with a new gradient each against torch.optim.Adam on float64 copies (lr 1e-3, betas (0.9, 0.999), eps 1e-8).
    The largest size is above the launcher's 8192 x 256 threads (grid-stride loop). Elements whose gradient is zero throughout must
    keep their value bit for bit. Compared: the parameter UPDATE p - p0 (parameters are about 0.05 in size, so their own f32 spacing
    stays 1e-6 of an update) and both moments. Bounds: MEASURED["adam ..."]."""
    p0 = rnd(W, 700, n % 1000, (n,), -0.05, 0.05)
    frozen = torch.zeros(n, dtype=torch.bool)
    frozen[::7] = True
    p, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    p64 = p0.double().requires_grad_(True)
    opt = torch.optim.Adam([p64], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    for step in range(1, 6):
        g = rnd(W, 700 + step, n % 1000, (n,), -1.0, 1.0) * (10.0 ** (step - 3))
        g[frozen] = 0.0
        ops.adam_step(p, g.cuda(), m, v, 1e-3, 0.9, 0.999, 1e-8, step)
        p64.grad = g.double()
        opt.step()
    st = opt.state[p64]
    assert torch.equal(p.cpu()[frozen], p0[frozen]), "a zero gradient must leave the parameter unchanged"
    measured("adam update", rel(p.cpu().double() - p0.double(), p64.detach() - p0.double()))
    measured("adam m", rel(m, st["exp_avg"]))
    measured("adam v", rel(v, st["exp_avg_sq"]))


def test_adam_step_and_axpy_on_zero_elements_touch_nothing(ops):
    one = [torch.full((1,), float(i + 1), device="cuda") for i in range(4)]
    L, s = ops._lib.lib(), ops._lib.stream_ptr()
    assert L.mla_adam_step(ops._p(one[0]), ops._p(one[1]), ops._p(one[2]), ops._p(one[3]), 0, 1e-3, 0.9, 0.999, 1e-8, 1, s) == 0
    assert L.mla_axpy(2.0, ops._p(one[0]), ops._p(one[1]), 0, s) == 0
    assert [float(t) for t in one] == [1.0, 2.0, 3.0, 4.0]


@pytest.mark.parametrize("n", SIZES)
def test_axpy_is_exact(ops, W, n):
    """y += a x is either two f32 operations (product rounded, then the sum) or one fused multiply-add (one rounding): the compiler
    may contract the expression, so EITHER form is accepted -- but the whole tensor must be exactly one of them. The fused
    form is evaluated in extended precision (the product of two f32 values is exact there)."""
    x, y = rnd(W, 710, n % 1000, (n,), -2.0, 2.0), rnd(W, 711, n % 1000, (n,), -2.0, 2.0)
    a = float(np.float32(0.3))
    got = ops.axpy(a, x.cuda(), y.cuda()).cpu().numpy()
    two = (y.numpy() + (np.float32(a) * x.numpy()).astype(np.float32)).astype(np.float32)
    fused = (y.numpy().astype(np.longdouble) + np.longdouble(a) * x.numpy().astype(np.longdouble)).astype(np.float32)
    assert n < 1000 or not np.array_equal(two, fused)                   # the two forms do differ on this data
    assert np.array_equal(got, two) or np.array_equal(got, fused)


@pytest.mark.parametrize("R,C,pitch", [(1, 1, 0), (33, 31, 0), (40, 128, 0), (77, 200, 0), (5120, 96, 0), (77, 50, 3)])
def test_transpose_padded_f32_is_exact(ops, W, R, C, pitch):
    """32 x 32 tiles through LDS: edge tiles in both directions, rows padded with zeros to a 16-byte pitch; one row-strided input."""
    x = rnd(W, 720, R, (R, C))
    t = ops.transpose_padded(strided(x, 1, pitch - 1) if pitch else x.cuda()).cpu()
    ld = (R + 3) // 4 * 4
    assert tuple(t.shape) == (C, ld) and torch.equal(t[:, :R], x.t()) and not bool(t[:, R:].any())
