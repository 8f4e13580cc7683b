"""GPU tests of the head beyond 16 classes: the wide attention-pooling kernels (one workgroup per bag, T <= 64, K <= 1024), the
column-mode BatchNorm above 64 channels, the composed head at 50 and 527 classes against the oracle in float64, and the training
step of an Ensemble(classes=50).

Bounds follow tests/test_train_kernels_gpu.py:
  derived   double-precision sums of f32 data and f32 chains without transcendental functions: per element, from the float64
            reference (bn_reference's count for the backward; the statistics' count is in the test that uses it);
  measured  kernels with __expf / the fast sigmoid: worst max|got - ref| / max|ref| over the whole parametrization as measured on
            the MI355X, times 4, never looser than the composed head test (1e-4 on outputs, 2e-3 on gradients): MEASURED below.
"""

import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PKG

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # unit roundoff of float32
EPS = 1e-5                # ops.BN_EPS
CAP_OUT, CAP_GRAD = 1e-4, 2e-3

# name -> worst relative error measured on the MI355X over the test's whole parametrization; the bound is 4 x that, capped (every
# bound here is far below its cap). The worst attention figures come from the spread-60 case (10, 527, 3) and from (64, 1024, 2).
# The BatchNorm figures also pass the derived per-element bounds of bn_reference, which are the sharper check.
MEASURED = {
    "wide attention y": 7.06e-7, "wide attention att": 1.32e-6, "wide attention cla": 1.18e-7,
    "wide attention du_v": 1.50e-6, "wide attention du_f": 3.86e-7,
    "wide bn dx": 3.16e-7, "wide bn dgamma": 1.84e-7, "wide bn dbeta": 6.57e-8,
}


def bound_of(name):
    cap = CAP_GRAD if " d" in name else CAP_OUT                 # du_v, du_f, dx, dgamma, dbeta are gradients
    return min(4 * MEASURED[name], cap)


def measured(name, err):
    """Print the figure, then assert it against the table."""
    print("MEASURE %s: %.3g (recorded %s, bound %.3g)" % (name, err, MEASURED[name], bound_of(name)))
    assert err < bound_of(name), (name, err)


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def M():
    return importlib.import_module(PKG + ".model")


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
    (10, 17, 3, 5.0), (17, 10, 3, 5.0), (10, 50, 17, 5.0), (10, 527, 5, 5.0), (10, 527, 3, 60.0), (33, 65, 2, 5.0),
    (64, 1024, 2, 5.0), (1, 1024, 1, 5.0), (64, 1, 2, 5.0)]


def _attention_inputs(W, T, K, bags, spread):
    seed = 300 + T * 17 + K
    z = rnd(W, seed, 1, (bags, T, K), -2.0, 2.0)        # |normalised z| <= 2.6 / sqrt(4 / 6) = 3.2
    nv = (rnd(W, seed, 2, (T,), -0.6, 0.6), rnd(W, seed, 3, (T,), 0.5, 2.0) * 4 / 3, rnd(W, seed, 4, (T,), 0.5, 1.5) * spread / 4.8,
          rnd(W, seed, 5, (T,), -0.5, 0.5))
    nf = (rnd(W, seed, 6, (T,), -0.6, 0.6), rnd(W, seed, 7, (T,), 0.5, 2.0) * 4 / 3, rnd(W, seed, 8, (T,), 0.5, 1.5),
          rnd(W, seed, 9, (T,), -0.5, 0.5))
    dy = rnd(W, seed, 10, (bags, K))
    return z, nv, nf, dy


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


def _run_pool(ops, z, nv, nf, dy, T, K, save=True):
    """Forward into a column slice between sentinels, backward from a strided dy."""
    bags = z.shape[0]
    zc = z.reshape(bags * T, K).cuda()
    nvc, nfc = [p.cuda() for p in nv], [p.cuda() for p in nf]
    ybuf = torch.full((bags, K + 5), -7.25, device="cuda")
    att, cla = ops.attention_pool(zc, bags, T, K, nvc, nfc, ybuf[:, 2:2 + K], save=save)
    if not save:
        return ybuf, att, cla, None, None
    du_v, du_f = ops.attention_pool_bwd(strided(dy), att, cla, bags, T, K)
    return ybuf, att, cla, du_v, du_f


@pytest.mark.parametrize("T,K,bags,spread", ATT_CASES)
def test_wide_attention_pool_and_its_backward_match_float64(ops, W, T, K, bags, spread):
    """mla_attention_pool / mla_attention_pool_bwd past the register kernels (T > 16 or K > 16): one workgroup per bag, rows by
    waves and columns by threads. First K and first T past the narrow kernel, K below / across / far above a wave and a block
    (50, 65, 527, 1024), T not a multiple of the four waves (10, 17, 33), both limits at once, a single row, a single column.
    y goes into a column slice (ldy > K; the rest keeps its sentinel), save=True and save=False give the same bits, spread 60
    exercises the max subtraction. Backward from the SAVED att / cla and a strided dy against float64 autograd w.r.t. the two
    BatchNorm outputs. Bounds: MEASURED["wide attention ..."]."""
    assert T > 16 or K > 16
    z, nv, nf, dy = _attention_inputs(W, T, K, bags, spread)
    u_v, u_f, att64, cla64, y64 = _attention_reference(z, nv, nf, T)
    # the inputs, not the kernel: |u_v| <= 2.6 * 1.23 * 1.5 * spread / 4.8 + 0.5 always; only the spread-60 case (ten slots) is
    # required to reach the range that needs the max subtraction
    top = float(u_v.detach().abs().max())
    assert top <= spread + 0.5 and (spread < 60.0 or top > 0.5 * spread), top
    ybuf, att, cla, du_v, du_f = _run_pool(ops, z, nv, nf, dy, T, K)
    ybuf2, none_a, none_c, _, _ = _run_pool(ops, z, nv, nf, dy, T, K, save=False)
    assert none_a is None and none_c is None
    assert torch.equal(ybuf, ybuf2), "y must not depend on whether att / cla are saved"
    assert bool((ybuf[:, :2] == -7.25).all()) and bool((ybuf[:, 2 + K:] == -7.25).all()), "columns outside the slice were written"
    assert bool(torch.isfinite(ybuf).all())
    measured("wide attention y", rel(ybuf[:, 2:2 + K], y64))
    measured("wide attention att", rel(att.reshape(bags, T, K), att64))
    measured("wide attention cla", rel(cla.reshape(bags, T, K), cla64))
    y64.backward(dy.double())
    if T == 1:
        # one time slot: y = cla, so d y / d u_v is identically zero; float64 autograd returns its own rounding noise, which is no
        # scale to divide by: the error is taken relative to the terms that cancel, dy * att / sum_t att = dy
        assert float(u_v.grad.abs().max()) < 1e-14
        measured("wide attention du_v", float((du_v.reshape(bags, T, K).double().cpu() - u_v.grad).abs().max()) / float(dy.abs().max()))
    else:
        measured("wide attention du_v", rel(du_v.reshape(bags, T, K), u_v.grad))
    measured("wide attention du_f", rel(du_f.reshape(bags, T, K), u_f.grad))


def test_wide_attention_bags_do_not_depend_on_their_batch(ops, W):
    """The same 5 bags of 10 x 527 alone and as bags 7..11 of 21: y, du_v and du_f bit for bit (every reduction's order depends on
    (T, K) only)."""
    T, K = 10, 527
    z, nv, nf, dy = _attention_inputs(W, T, K, 21, 5.0)
    yb, _, _, du_v, du_f = _run_pool(ops, z, nv, nf, dy, T, K)
    ys, _, _, sv, sf = _run_pool(ops, z[7:12].contiguous(), nv, nf, dy[7:12].contiguous(), T, K)
    assert torch.equal(yb[7:12], ys)
    assert torch.equal(du_v.reshape(21, T, K)[7:12], sv.reshape(5, T, K))
    assert torch.equal(du_f.reshape(21, T, K)[7:12], sf.reshape(5, T, K))


def test_attention_pool_refuses_more_than_64_slots_or_1024_classes(ops):
    L = importlib.import_module(PKG + "._lib")
    for T, K in ((65, 10), (10, 1025)):
        z = torch.zeros(T, K, device="cuda")
        p = [torch.ones(T, device="cuda")] * 4
        y = torch.zeros(1, K, device="cuda")
        with pytest.raises(L.MlaError) as e:
            ops.attention_pool(z, 1, T, K, p, p, y)
        assert e.value.code == -2                                   # MLA_E_SHAPE
        with pytest.raises(L.MlaError) as e:
            ops.attention_pool_bwd(y, z, z, 1, T, K)
        assert e.value.code == -2


# ------------------------------------------------------------------------------------ column-mode BatchNorm ----

WIDE_COLS = (65, 527, 1024)       # one column past sums_cols_kernel, nine column blocks with a ragged last one, the limit


def _stats_reference(x, run_mean, run_var, momentum):
    """float64 statistics per column and their bounds. The kernels add x and x^2 in double (exact to 2^-53 relative per addition:
    below 1e-12 of sum|x| / n and sum x^2 / n for these sizes), form mean and biased variance in double and round each ONCE to f32:
    |error| <= u |value| + 1e-12 (mean|x| or mean x^2). Running update in double with the f32 momentum 0.1f (2^-26 relative off
    0.1: at most 1.5e-9 (|old| + |stat|)), rounded once. One row: torch has no unbiased variance; the kernel keeps the biased 0."""
    x64 = x.double()
    n = x.shape[0]
    mean, var = x64.mean(0), x64.var(0, unbiased=False)
    unb = var * n / (n - 1) if n > 1 else var
    rm = (1 - momentum) * run_mean.double() + momentum * mean
    rv = (1 - momentum) * run_var.double() + momentum * unb
    b_mean = U * mean.abs() + 1e-12 * x64.abs().mean(0)
    b_var = U * var + 1e-12 * (x64 * x64).mean(0)
    scale = n / (n - 1) if n > 1 else 1.0
    return {"mean": mean, "var": var, "run_mean": rm, "run_var": rv,
            "b_mean": b_mean, "b_var": b_var,
            "b_run_mean": U * rm.abs() + momentum * b_mean + 1.5e-9 * (run_mean.double().abs() + mean.abs()),
            "b_run_var": U * rv.abs() + momentum * scale * b_var + 1.5e-9 * (run_var.double().abs() + unb.abs())}


@pytest.mark.parametrize("rows", [1, 7, 300])
@pytest.mark.parametrize("cols", WIDE_COLS)
def test_wide_column_statistics_match_float64(ops, W, rows, cols):
    """mla_bn_stats and mla_bn_stats_fused in mode 1 above 64 columns (sums_cols_wide_kernel: 64 columns x up to 32 row blocks per
    workgroup; 300 rows = 5 row blocks, the last one short), running statistics and num_batches_tracked included. The two entry
    points must give the same bits."""
    x = rnd(W, 700 + rows + cols, 1, (rows, cols), -1.0, 3.0)
    rm0, rv0 = rnd(W, 700 + cols, 2, (cols,), -0.5, 0.5), rnd(W, 700 + cols, 3, (cols,), 0.5, 2.0)
    ref = _stats_reference(x, rm0, rv0, 0.1)
    what = "bn_stats %dx%d " % (rows, cols)
    rm, rv = rm0.cuda(), rv0.cuda()
    mean, var = ops.bn_stats(x.cuda(), 1, 0, rm, rv, 0.1)
    for got, k in ((mean, "mean"), (var, "var"), (rm, "run_mean"), (rv, "run_var")):
        within(got, ref[k], ref["b_" + k], what + k)
    rm2, rv2, trk = rm0.cuda(), rv0.cuda(), torch.tensor(4, dtype=torch.int64, device="cuda")
    mean2, var2 = ops.bn_stats_sync(x.cuda(), 1, 0, ops._local(), rm2, rv2, 0.1, tracked=trk)
    assert int(trk) == 5
    for a, b in ((mean, mean2), (var, var2), (rm, rm2), (rv, rv2)):
        assert torch.equal(a, b), what + "fused form"


@pytest.mark.parametrize("cols", WIDE_COLS)
def test_wide_column_statistics_split_path_equals_one_call(ops, W, cols):
    """The data-parallel entry points in one process: mla_bn_stats_sums on two half-batches, the [2 x channels] double messages
    added on the host (what the all-reduce does), mla_bn_stats_finish with the global count -- against mla_bn_stats_fused on the
    whole batch. Sums of f32 data in double: the two orders differ by at most a few 2^-53 of sum|x| resp. sum x^2, far below the one
    f32 rounding of the result; bound: that rounding (u |value|) on top of the whole-batch result taken as exact."""
    L = importlib.import_module(PKG + "._lib")
    rows = 300
    x = rnd(W, 760 + cols, 1, (rows, cols), -1.0, 3.0).cuda()
    rm0, rv0 = rnd(W, 760 + cols, 2, (cols,), -0.5, 0.5), rnd(W, 760 + cols, 3, (cols,), 0.5, 2.0)
    rm, rv = rm0.cuda(), rv0.cuda()
    mean, var = ops.bn_stats_sync(x, 1, 0, ops._local(), rm, rv, 0.1)
    lib, p, ws = L.lib(), ops._p, ops._workspace(x.device)
    total = torch.zeros(2 * cols, dtype=torch.float64, device="cuda")
    for lo, hi in ((0, 137), (137, rows)):                        # unequal halves: the count travels with the finish
        part = torch.empty(2 * cols, dtype=torch.float64, device="cuda")
        half = x[lo:hi]
        L.check(lib.mla_bn_stats_sums(p(half), hi - lo, cols, half.stride(0), 1, 0, p(ws), p(part), L.stream_ptr()))
        total += part
    mean2, var2 = torch.empty_like(mean), torch.empty_like(var)
    rm2, rv2 = rm0.cuda(), rv0.cuda()
    L.check(lib.mla_bn_stats_finish(p(total), cols, float(rows), p(mean2), p(var2), p(rm2), p(rv2), 0.1, None, L.stream_ptr()))
    ref = _stats_reference(x.cpu(), rm0, rv0, 0.1)
    for got, k in ((mean2, "mean"), (var2, "var"), (rm2, "run_mean"), (rv2, "run_var")):
        within(got, ref[k], ref["b_" + k], "split bn_stats %d cols %s" % (cols, k))
    for a, b, k in ((mean, mean2, "mean"), (var, var2, "var"), (rm, rm2, "run_mean"), (rv, rv2, "run_var")):
        within(b, a.double().cpu(), 2 * U * a.double().cpu().abs() + 1e-12, "split vs one call %d cols %s" % (cols, k))


def _bn_channels(t, mode, period):
    """View with the channel on axis 1 and everything reduced on axes 0 and 2."""
    rows, cols = t.shape
    return t.reshape(rows // period, period, cols) if mode == 0 else t.reshape(rows, cols, 1)


def bn_reference(x, dy, gamma, beta, mode, period, act, keep, drop_scale, stats=None):
    """float64 autograd through y = act((x - mean) rsqrt(var + eps) gamma + beta) [* keep * drop_scale] with the batch statistics
    computed here (stats=None) or FIXED statistics (mean, var). Returns the forward output, the three gradients and the derived
    per-element bounds; the rounding count is the one of tests/test_train_kernels_gpu.py (same apply kernel, same functors):
      xhat 7 roundings of u (|x| + |mean|) inv; g through the activation 0 / 1 / 4 roundings;
      dbeta (n_g + 1) u sum|g|; dgamma (n_g + 8) u sum |g| (|x| + |mean|) inv; dx 28 u |gamma| inv (|g| + A + span B)."""
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
            "var": var.detach().reshape(-1).float(), "bounds": bounds}


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("rows", [7, 300])
@pytest.mark.parametrize("cols", WIDE_COLS)
def test_wide_column_bn_backward_matches_float64_autograd(ops, W, cols, rows, act):
    """mla_bn_bwd_sums + mla_bn_bwd_apply in mode 1 above 64 columns, plain and through the sigmoid the head's last BatchNorm is
    fused with, dense and as misaligned column slices; dgamma / dbeta above 256 channels take more than one trip of the writing
    block. Against float64 autograd on the reference's own forward output and statistics (rounded to f32): the derived per-element
    bounds of bn_reference, and the MEASURED relative figures."""
    x = rnd(W, 800 + rows + cols, 1, (rows, cols), -1.0, 3.0)
    dy = rnd(W, 800 + rows + cols, 2, (rows, cols))
    gamma, beta = rnd(W, 800 + cols, 3, (cols,), 0.5, 1.5), rnd(W, 800 + cols, 4, (cols,), -0.5, 0.5)
    ref = bn_reference(x, dy, gamma, beta, 1, 0, act, None, 1.0)
    for layout, put in (("dense", lambda t: t.cuda()), ("strided", strided)):
        what = "bn_backward mode 1 %dx%d act %d %s" % (rows, cols, act, layout)
        dgamma, dbeta = torch.full((cols,), 9.0, device="cuda"), torch.full((cols,), 9.0, device="cuda")
        yout = put(ref["y"].float()) if act else None
        dx = ops.bn_backward(put(x), put(dy), yout, act, 1.0, 1, 0, ref["mean"].cuda(), ref["var"].cuda(), gamma.cuda(), ops._local(),
                             dgamma, dbeta)
        for got, k in ((dx, "dx"), (dgamma, "dgamma"), (dbeta, "dbeta")):
            within(got, ref[k], ref["bounds"][k], what + " " + k)
            measured("wide bn " + k, rel(got, ref[k]))


# ------------------------------------------------------------------------------------------- composed head ----

def _masks(W, seed, conf, B, slots, hidden, prefix="mla."):
    out = {}
    for lvl, n_fc in enumerate(conf):
        for j in range(n_fc):
            key = "%sembedded_mappings.%d.dropouts.%d" % (prefix, lvl, j)
            out[key] = torch.as_tensor(W.keep_mask(seed, W.stream_id(key), B * slots * hidden, 0.4)).reshape(B, slots, hidden)
    return out


def _install(mla, masks, prefix="mla."):
    for lvl, em in enumerate(mla.embedded_mappings):
        for j, d in enumerate(em.dropouts):
            d.mask = masks["%sembedded_mappings.%d.dropouts.%d" % (prefix, lvl, j)]


HEADS = [dict(classes=50), dict(classes=527, slots=12, hidden=64)]
STATS = ("running_mean", "running_var", "num_batches_tracked")


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("kw", HEADS, ids=["k50", "k527-t12-h64"])
def test_wide_head_matches_the_oracle_in_float64(M, W, kw, train):
    """MultiLevelAttention([2, 1], 128, ...) at 50 classes (default slots / hidden) and at 527 classes x 12 slots x 64 hidden, 6
    bags, eval mode (running statistics away from their initial values) and train mode (batch statistics, injected masks), through
    HeadFn: the output, the running statistics after the train-mode forward, the input gradient and every parameter gradient
    against float64 autograd through oracle.model.mla_forward on the same state_dict. fcf receives no gradient. Tolerances: what
    the composed head tests grant (1e-4 outputs, 2e-3 gradients, floors as in test_head_gradients_match_the_oracle_autograd)."""
    from oracle import model as omodel
    conf, B = [2, 1], 6
    K, T, H = kw.get("classes", 10), kw.get("slots", 10), kw.get("hidden", 600)
    sd = W.make_state_dict(3, W.mla_shapes(conf, 128, prefix="mla.", T=T, H=H, K=K))
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = W.uniform(5, W.stream_id(k), sd[k].size, lo=-0.5, hi=0.5).astype(np.float32).reshape(sd[k].shape)
        if k.endswith("running_var"):
            sd[k] = W.uniform(5, W.stream_id(k), sd[k].size, lo=0.5, hi=2.0).astype(np.float32).reshape(sd[k].shape)
    x = torch.from_numpy(W.uniform(4, W.stream_id("mla_in/m128"), B * T * 128, lo=0.0, hi=2.0)).reshape(B, T, 128)
    wgt = torch.from_numpy(W.uniform(4, W.stream_id("loss_w"), B * K, lo=-1.0, hi=1.0)).reshape(B, K)
    masks = _masks(W, 5, conf, B, T, H) if train else None
    ref_sd = {k: (torch.as_tensor(v).double() if not k.endswith("num_batches_tracked") else torch.as_tensor(v)).clone()
              .requires_grad_(not k.endswith(STATS) and ".fcf." not in k) for k, v in sd.items()}
    xr = x.double().requires_grad_(True)
    stats = {} if train else None
    ref = omodel.mla_forward(ref_sd, xr, tuple(conf), train=train, masks=masks, stats_out=stats)
    (ref * wgt.double()).sum().backward()

    mla = M.MultiLevelAttention(conf, 128, **kw)
    mla.load_state_dict({k[len("mla."):]: torch.as_tensor(v) for k, v in sd.items()})
    mla.cuda().train(train)
    if train:
        _install(mla, masks)
    xg = x.cuda().requires_grad_(True)
    out = mla(xg)
    assert tuple(out.shape) == (B, K) and out.requires_grad
    err = rel(out, ref)
    print("MEASURE head %s train=%s out: %.3g" % (kw, train, err))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=CAP_OUT, atol=1e-6)
    if train:
        buf = mla.state_dict()
        for key, (mean, unbiased) in stats.items():
            name = key[len("mla."):]
            for leaf, stat in (("running_mean", mean), ("running_var", unbiased)):
                want = 0.9 * torch.as_tensor(sd[key + "." + leaf]).double() + 0.1 * stat
                np.testing.assert_allclose(buf[name + "." + leaf].cpu().numpy(), want.numpy(), rtol=CAP_OUT, atol=1e-6, err_msg=key)
            assert int(buf[name + ".num_batches_tracked"]) == 1, key
    (out * wgt.cuda()).sum().backward()
    scale = float(xr.grad.abs().max())
    print("MEASURE head %s train=%s dx: %.3g" % (kw, train, rel(xg.grad, xr.grad)))
    np.testing.assert_allclose(xg.grad.cpu().numpy(), xr.grad.numpy(), rtol=CAP_GRAD, atol=2e-5 * scale)
    # mathematically zero gradients (biases in front of a train-mode BatchNorm, normv.bias under the softmax's shift invariance) are
    # f32 rounding noise here and f64 rounding noise there: an absolute floor of 2e-5 of the model's largest gradient entry
    floor = 2e-5 * max(float(v.grad.abs().max()) for v in ref_sd.values() if v.grad is not None)
    for n, p in mla.named_parameters():
        r = ref_sd["mla." + n].grad
        if ".fcf." in n:
            assert p.grad is None and r is None
            continue
        s_ = float(r.abs().max())
        print("MEASURE head %s train=%s %s: %.3g" % (kw, train, n, rel(p.grad, r)))
        np.testing.assert_allclose(p.grad.cpu().numpy(), r.numpy(), rtol=CAP_GRAD, atol=2e-5 * s_ + floor, err_msg=n)


# ----------------------------------------------------------------------------------------------- TrainStep ----

CNN_CONF = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False,
                cnn_trainable=False, first_cnn_layer_trainable=False, in_channels=1)
ZERO_GRAD = ("fc.bias", "fc.0.bias", "fc.1.bias", "fcv.bias", "normv.bias")   # mathematically zero gradients: Adam steps on rounding noise
STEPS, BAGS, LR = 3, 4, 1e-3


def _bags(W, seed, classes):
    """(4, 10, 1, 96, 64) inputs in the front-end's value range; labels over all classes, the last one the highest class."""
    x = W.uniform(seed, W.stream_id("bags"), BAGS * 10 * 96 * 64, lo=-1.4, hi=4.6)
    y = W.bits24(seed, W.stream_id("labels"), BAGS) % classes
    y[-1] = classes - 1
    return torch.as_tensor(x).reshape(BAGS, 10, 1, 96, 64), torch.as_tensor(y.astype(np.int64))


def _ensemble50(M, W):
    torch.manual_seed(77)                                        # Dropout reads the seed at construction
    shapes = W.mla_shapes([2, 1], 128, prefix="mla.", K=50)
    shapes.update(W.vggish_shapes("cnn.cnn_model."))
    sd = W.make_state_dict(7, shapes)
    ens = M.Ensemble("repeat", dict(CNN_CONF), [2, 1], torch.device("cuda"), classes=50)
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return ens.cuda(), sd


def test_train_step_at_50_classes_matches_a_float64_restatement(M, W):
    """Frozen-VGGish Ensemble(classes=50), 4 bags, 3 eager steps with injected dropout masks against float64: oracle.mla_forward
    (train mode) + F.cross_entropy + torch.optim.Adam on the head's parameters (fcf excluded: no gradient), fed the model's own CNN
    features. Labels include 49 although cnn_conf["num_classes"] is 10; a host label 50 raises IndexError.
    Loss: 1e-4, the outputs' cap. Parameters: Adam moves an entry by about lr per step whatever the gradient's size, so a
    relative gradient error e moves an update by about lr e (2e-6 at the 2e-3 cap); entries whose gradient is itself rounding noise
    may go either way: 2 % of the possible travel lr x steps = 6e-5 absolute, 1e-3 relative. The mathematically-zero gradients
    (ZERO_GRAD) are left out as in the golden training tests. Measured on the MI355X: loss within 1.2e-7 relative at every step,
    worst parameter difference 5.88e-5 -- close to the 6e-5 (the test prints the tensor it sits in). The likely source, not
    verified: entries whose gradient is small against their tensor's largest carry the tensor-wide f32 error (about 1e-5 of the
    largest entry) as a percent-level relative error, which Adam's m / sqrt(v) passes on as that fraction of lr from step 2 on."""
    from oracle import model as omodel
    TR = importlib.import_module(PKG + ".train")
    ens, sd = _ensemble50(M, W)
    assert ens.num_classes == 10 and ens.mla.classes == 50
    step = TR.TrainStep(ens, lr=LR, graph=False)
    ref_sd = {k: (torch.as_tensor(v).double() if v.dtype != np.int64 else torch.as_tensor(v)).clone() for k, v in sd.items() if k.startswith("mla.")}
    train_keys = [k for k in ref_sd if not k.endswith(STATS) and ".fcf." not in k]
    for k in train_keys:
        ref_sd[k].requires_grad_(True)
    opt = torch.optim.Adam([ref_sd[k] for k in train_keys], lr=LR)
    for s in range(STEPS):
        x, y = _bags(W, 100 + s, 50)
        assert int(y.max()) == 49
        masks = _masks(W, 200 + s, [2, 1], BAGS, 10, 600)
        _install(ens.mla, masks)
        with torch.no_grad():
            feats = ens.cnn(ens.input(x.cuda())).reshape(BAGS, 10, 128).double().cpu()
        loss, hits = step(x.cuda(), y if s % 2 else y.cuda())     # host and device labels alternate
        opt.zero_grad()
        ref_loss = F.cross_entropy(omodel.mla_forward(ref_sd, feats, (2, 1), train=True, masks=masks), y)
        ref_loss.backward()
        opt.step()
        ref_loss = float(ref_loss.detach())
        print("MEASURE trainstep loss step %d: %.3g" % (s, abs(float(loss) - ref_loss) / ref_loss))
        assert float(loss) == pytest.approx(ref_loss, rel=CAP_OUT), s
        assert int(hits[1]) == 0
    got = ens.state_dict()
    worst = (0.0, None)
    for k in train_keys:
        if k.endswith(ZERO_GRAD):
            continue
        worst = max(worst, (float((got[k].double().cpu() - ref_sd[k].detach()).abs().max()), k))
        np.testing.assert_allclose(got[k].cpu().numpy(), ref_sd[k].detach().numpy(), rtol=1e-3, atol=0.02 * LR * STEPS, err_msg=k)
    print("MEASURE trainstep worst parameter |difference|: %.3g in %s" % worst)
    assert torch.equal(got["mla.attention_modules.0.fcf.weight"].cpu(), torch.as_tensor(sd["mla.attention_modules.0.fcf.weight"]))
    # labels are checked against the head's classes, not cnn_conf["num_classes"]
    x, y = _bags(W, 100, 50)
    y[0] = 50
    with pytest.raises(IndexError, match="Target 50 is out of bounds"):
        step(x.cuda(), y)
    assert step.t == STEPS


def test_train_step_graph_equals_eager_at_50_classes(M, W):
    """The step as one HIP graph against the same steps run eagerly, masks drawn on the device: losses, hit counts, every updated
    parameter, the Adam moments and the running statistics bit for bit, as test_graph_replays_equal_eager_steps requires for the
    default head. The wide pooling and BatchNorm kernels are captured (no allocation, no host sync inside)."""
    TR = importlib.import_module(PKG + ".train")
    runs, ords = [], None
    for graph in (False, True):
        ens, _ = _ensemble50(M, W)
        drops = [m for m in ens.mla.modules() if type(m).__name__ == "Dropout"]
        if ords is None:
            ords = [d.ordinal for d in drops]
        for d, o in zip(drops, ords):                              # the mask stream is keyed by the module's ordinal: same for both
            d.ordinal = o
        step = TR.TrainStep(ens, lr=LR, graph=graph)
        out = []
        for s in range(STEPS):
            x, y = _bags(W, 100 + s, 50)
            loss, hits = step(x.cuda(), y.cuda() if s % 2 else y)
            out.append((float(loss), hits.tolist()))
        assert (step._graph is not None) == graph and step.t == STEPS
        runs.append((out, step, ens))
    (ref, step_e, ens_e), (got, step_g, ens_g) = runs
    assert got == ref, (got, ref)
    assert torch.equal(step_g.flat_p, step_e.flat_p) and torch.equal(step_g.flat_m, step_e.flat_m) and torch.equal(step_g.flat_v, step_e.flat_v)
    for (k, a), (_, b) in zip(ens_g.state_dict().items(), ens_e.state_dict().items()):
        assert torch.equal(a, b), k
