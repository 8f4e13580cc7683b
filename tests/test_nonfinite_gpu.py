"""NaN and Inf through every compute kernel, one kernel call at a time, against float64 torch / numpy of the same stored operands.

The rule (tests/nonfinite_cases.py same_nonfinite): the NaN positions of a kernel's output equal the reference's, +inf and -inf
sit exactly where the reference has them, and the finite rest meets the criterion of the kernel's existing finite test. It fails a
kernel that drops a NaN (fmaxf(x, 0) gives 0 where nn.ReLU, nn.MaxPool2d, torch.clamp and np.maximum give NaN) and one that leaks
one out of memory the result must not depend on (an operand masked by a product with 0 instead of being skipped). Operands, shapes
and criteria are those of the sibling finite tests, at their smallest shape that still has a tile tail and two images or row
tiles; the injection patterns a .. e are described in nonfinite_cases.py.

The gradient masks of the backward kernels (a > 0 ? d : 0, the arg-max routing of the pools, the window codes) are deliberately
NOT torch's threshold_backward on NaN activations; section 9 pins what they do today.
"""

import ctypes
import importlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import infer_kernel_cases as K
import nonfinite_cases as N
from conftest import PKG
from infer_kernel_cases import BF16, F32, name
from nonfinite_cases import INF, NAN, same_bits, same_nonfinite

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
SENTINEL = -7.0


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def code(L, dtype):
    return L.F32 if dtype == F32 else L.BF16


def ptr(t):
    return vp(t.data_ptr()) if t is not None else None


def nan_like(shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------- 1. VGGish inference convs ----

@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16x3"])
@pytest.mark.parametrize("layer", K.LAYERS)
def test_vggish_conv(ops, layer, mode):
    """mla_vggish_conv at 5 images (a tail in the 4-image W = 8 tiles and in the image pairs of the 2 x 4-wave tiles), every
    pattern one launch. Finite criterion: test_conv_small_batch_is_exact's bit-equality on the grid (bf16x3: plane by plane). e: the
    five images are the head of a six-image allocation whose last image is NaN."""
    x3 = mode == "bf16x3"
    case = K.conv_case(layer, "sparse9" if x3 else "grid")
    n, pool = K.SMALL_N, case["g"]["pool"]
    dtype = F32 if mode == "f32" else BF16

    def run(x, w, b):
        xs, wp = N.conv_stored(x, w, mode)
        return ops.conv(layer, xs.cuda()[:n], wp.cuda(), b.cuda(), split=x3)

    clean = run(case["x"][:n], case["w"], case["b"])
    assert bool(torch.isfinite(clean.float()).all())
    for pattern in N.CONV_PATTERNS:
        what = "conv%d %s %s" % (layer, mode, pattern)
        x, w, b, keep, channel = N.conv_inject(case, pattern, n)
        got = run(x, w, b)
        ref, _ = N.conv_reference(x[:n], w, b, pool, x3)
        assert bool((~torch.isfinite(ref)).any()) == (pattern != "e"), what
        if x3:
            fin = same_nonfinite(N.merged(got), ref, what, x3_inf=pattern == "c")
            N.assert_split_planes(got, ref, fin, what)
        else:
            same_nonfinite(got, ref, what, finite=N.exact(dtype))
        assert same_bits(got[keep], clean[keep]), what + ": an image the pattern does not touch changed"
        if channel is not None:
            N.assert_channels(ref, channel, what)


def conv1_inject(case, pattern, n):
    x, w, b = case["x"][:n].clone(), case["w"].clone(), case["b"].clone()
    keep, channel = slice(0, 0), None
    if pattern == "a":
        x[0, 40, 30] = NAN
        keep = slice(1, n)
    elif pattern == "b":
        x[n - 1, 95, 63] = NAN
        keep = slice(0, n - 1)
    elif pattern == "c":
        x[0, 1, 1], x[n - 1, 94, 62] = INF, -INF
        keep = slice(1, n - 1)
    elif pattern == "d-weight":
        channel = 61
        w[channel, 0, 1, 1] = NAN
    elif pattern == "d-bias":
        channel = 1
        b[channel] = NAN
    else:
        x = torch.cat([x, torch.full_like(x[:1], NAN)])
        keep = slice(0, n)
    return x, w, b, keep, channel


@pytest.mark.parametrize("pattern", N.CONV_PATTERNS)
@pytest.mark.parametrize("pair", K.CONV1_PAIRS, ids=lambda p: "%s-%s" % (name(p[0]), name(p[1])))
def test_vggish_conv1(ops, pair, pattern):
    """mla_vggish_conv1 at 3 clips on the grid operands of test_conv1_is_exact (bit-equality).

    Pattern c with a bf16 OUTPUT is the leak case of this kernel (conv1_patch_kernel, also the body of the fused front-end): it
    multiplies one 4 x 4 input patch with four zero-padded copies of the filter, one per position of the pooling window, so an Inf at
    the edge of a patch meets a padded 0 in the positions that do not read it. Unmasked, 0 * inf = NaN turned 342 outputs into NaN
    where the reference has +inf (relu(max(.., +inf))) or a finite value (max(.., -inf)); conv1_core.h now zeroes the unread patch
    elements per position in the (wave-uniform, rare) case that a patch holds an Inf or NaN."""
    x_dtype, out_dtype = pair
    case = K.conv1_case("grid")
    n = 3
    clean = ops.conv1(case["x"][:n].to(x_dtype).cuda(), case["w"].cuda(), case["b"].cuda(), out_dtype)
    x, w, b, keep, channel = conv1_inject(case, pattern, n)
    got = ops.conv1(x.to(x_dtype).cuda()[:n], w.cuda(), b.cuda(), out_dtype)
    ref, ref_abs = K.conv1_reference(x[:n], w, b)
    K.assert_exact_arithmetic(torch.nan_to_num(ref_abs, nan=0.0, posinf=0.0, neginf=0.0))
    what = "conv1 %s->%s %s" % (name(x_dtype), name(out_dtype), pattern)
    same_nonfinite(got, ref, what, finite=N.exact(out_dtype))
    assert same_bits(got[keep], clean[keep]), what
    if channel is not None:
        N.assert_channels(ref, channel, what)


def test_logmel_conv1_with_a_nan_sample(ops, fe, W):
    """The fused front-end (mla_logmel_conv1, bf16): a NaN sample in waveform 0 gives the bits of conv1(waveforms_to_examples(.))
    (the existing fused test's criterion), NaN where the float64 chain oracle log-mel -> conv1 has NaN, and the other waveform
    keeps the clean run's bits."""
    from oracle import frontend as ofe
    n_wave, n_samples = 2, 2 * 15360 + 240
    pcm = W.waveform(11, n_samples, n_wave).astype(np.float32)
    gen = torch.Generator().manual_seed(5)
    w, b = (torch.rand((64, 1, 3, 3), generator=gen) - 0.5).cuda(), (torch.rand((64,), generator=gen) - 0.5).cuda()
    clean = ops.logmel_conv1(torch.from_numpy(pcm).cuda(), w, b)
    bad = N.nan_sample(pcm, (0, 20000))
    got = ops.logmel_conv1(torch.from_numpy(bad).cuda(), w, b)
    two = ops.conv1(fe.waveforms_to_examples(torch.from_numpy(bad).cuda(), BF16), w, b, BF16)
    assert same_bits(got, two)
    n_ex = got.shape[0] // n_wave
    assert same_bits(got[n_ex:], clean[n_ex:]), "the other waveform changed"
    ex = torch.from_numpy(ofe.batch_examples(bad.astype(np.float64)))
    ref, _ = K.conv1_reference(ex, w.cpu(), b.cpu())
    assert bool(torch.isnan(ref).any()) and not bool(torch.isnan(ref[n_ex:]).any())
    same_nonfinite(got, ref, "logmel_conv1 with a NaN sample")


# ------------------------------------------------------------------------------------------------- 2. GEMM ----

GEMM_PATTERNS = ("a", "b", "c", "d-weight", "d-bias")


def gemm_inject(a, w, b, pattern):
    """-> a, w, b (copies), the rows that must keep the clean run's bits, the poisoned column."""
    a, w, b = a.clone(), w.clone(), None if b is None else b.clone()
    M, kk = a.shape
    keep = torch.ones(M, dtype=torch.bool, device=a.device)
    column = None
    if pattern == "a":
        a[1, kk // 2] = NAN
        keep[1] = False
    elif pattern == "b":
        a[M - 1, kk - 1] = NAN
        keep[M - 1] = False
    elif pattern == "c":
        a[0, 0], a[M - 1, 1] = INF, -INF
        keep[0] = keep[M - 1] = False
    elif pattern == "d-weight":
        column = w.shape[0] - 2
        w[column, kk // 2] = NAN
        keep[:] = False
    elif pattern == "d-bias":
        column = 1
        b[column] = NAN
        keep[:] = False
    else:
        raise KeyError(pattern)
    return a, w, b, keep, column


def check_gemm(run, reference, a, w, b, out_dtype, what, x3=False, relus=(True, False)):
    """run(a, w, b, relu) -> (M, N) output of f32-valued operands; reference(a, w, b) -> float64 (y, sum|terms|). Every pattern with
    and without ReLU against the exact criterion of the dyadic-grid tests."""
    clean = {relu: run(a, w, b, relu) for relu in relus}
    y, y_abs = reference(a, w, b)
    K.assert_exact_arithmetic(y_abs, 2.0 ** -18 if x3 else 2.0 ** -6)
    for relu in relus:
        same_nonfinite(clean[relu], F.relu(y) if relu else y, what + " clean", finite=N.exact(out_dtype))
    for pattern in GEMM_PATTERNS:
        a2, w2, b2, keep, column = gemm_inject(a, w, b, pattern)
        y, _ = reference(a2, w2, b2)
        assert bool((~torch.isfinite(y)).any())
        if column is not None:
            N.assert_channels(y, column, what + " " + pattern)
        for relu in relus:
            tag = "%s %s relu=%d" % (what, pattern, relu)
            got = run(a2, w2, b2, relu)
            keep = keep.to(got.device)
            same_nonfinite(got, F.relu(y) if relu else y, tag, finite=N.exact(out_dtype), x3_inf=x3 and pattern == "c")
            assert same_bits(got[keep], clean[relu][keep]), tag + ": a row the pattern does not touch changed"
    return clean


def padded(t, rows_behind, cols_behind, dtype):
    """t as the head of a NaN-filled allocation: `rows_behind` rows and `cols_behind` columns (the pitch) of NaN around it."""
    buf = nan_like((t.shape[0] + rows_behind, t.shape[1] + cols_behind), dtype)
    buf[:t.shape[0], :t.shape[1]] = t.to(dtype)
    return buf


@pytest.mark.parametrize("pair", [(F32, F32), (BF16, BF16)], ids=lambda p: "%s-%s" % (name(p[0]), name(p[1])))
@pytest.mark.parametrize("case_id", list(K.GEMM_CASES))
def test_linear_forms(ops, L, cus, case_id, pair):
    """mla_linear in every tile form of GEMM_CASES (asserted with the device's CU count), patterns a .. d through ops.linear with and
    without ReLU; e through the library: a, w and out with pitches, the padding of a and w, two rows behind M and one behind N all
    NaN -- the output keeps the clean run's bits and its own padding."""
    dtype, out_dtype = pair
    M, Nn, _ = K.GEMM_CASES[case_id]
    kk = K.gemm_k(case_id, dtype)
    form = K.gemm_form(M, Nn, kk, K.KPR[dtype], cus)
    assert form == K.form_of(case_id), "on %d CUs this case runs the %s form" % (cus, form)
    a, w, b = K.gemm_operands(M + Nn + kk, M, Nn, kk, device="cuda")
    run = lambda a_, w_, b_, relu: ops.linear(a_.to(dtype), w_.to(dtype), b_, relu=relu, out_dtype=out_dtype)       # noqa: E731
    clean = check_gemm(run, K.gemm_reference, a, w, b, out_dtype, "linear %s %s" % (case_id, name(dtype)))
    lda, ldw, ldo = kk + 3 * K.PER[dtype], kk + K.PER[dtype], Nn + 5
    ap, wp = padded(a, 2, lda - kk, dtype), padded(w, 1, ldw - kk, dtype)
    for relu in (True, False):
        out = torch.full((M + 1, ldo), SENTINEL, dtype=out_dtype, device="cuda")
        L.check(L.lib().mla_linear(ptr(ap), lda, ptr(wp), ldw, ptr(b), ptr(out), ldo, M, Nn, kk, code(L, dtype), code(L, out_dtype), int(relu),
                                   L.stream_ptr()))
        assert same_bits(out[:M, :Nn], clean[relu]), "e: NaN padding reached the output (relu=%d)" % relu
        assert bool((out[:M, Nn:] == SENTINEL).all()) and bool((out[M] == SENTINEL).all())


@pytest.mark.parametrize("pair", [(F32, F32), (BF16, BF16)], ids=lambda p: "%s-%s" % (name(p[0]), name(p[1])))
def test_linear_ksplit(L, pair):
    """mla_linear_ksplit, 133 x 100 with three 128-byte rows per range (test_linear_ksplit_is_exact's shape): the workspace starts as
    NaN in every run; e adds pitches, NaN padding and NaN rows behind M and N."""
    dtype, out_dtype = pair
    M, Nn, S = 133, 100, K.C["ksplit"]
    kk = K.KPR[dtype] * S * 3
    a, w, b = K.gemm_operands(M + 3, M, Nn, kk, device="cuda")

    def launch(ap, lda, wp, ldw, b_, relu):
        out, ws = torch.full((M, Nn), SENTINEL, dtype=out_dtype, device="cuda"), nan_like((S * M * Nn,))
        L.check(L.lib().mla_linear_ksplit(ptr(ap), lda, ptr(wp), ldw, ptr(b_), ptr(out), Nn, M, Nn, kk, code(L, dtype), code(L, out_dtype),
                                          int(relu), S, ptr(ws), ws.numel(), L.stream_ptr()))
        return out

    run = lambda a_, w_, b_, relu: launch(a_.to(dtype), kk, w_.to(dtype), kk, b_, relu)                # noqa: E731
    clean = check_gemm(run, K.gemm_reference, a, w, b, out_dtype, "linear_ksplit %s" % name(dtype))
    pad = 8
    for relu in (True, False):
        got = launch(padded(a, 2, pad, dtype), kk + pad, padded(w, 1, pad, dtype), kk + pad, b, relu)
        assert same_bits(got, clean[relu]), "e (relu=%d)" % relu


def test_linear_splitk(L):
    """mla_linear_splitk (f32), 133 x 100 x 768 in 2 ranges through the library: NaN workspace, then NaN pitches and rows (e)."""
    M, Nn, kk, splits = 133, 100, 768, 2
    a, w, b = K.gemm_operands(kk, M, Nn, kk, device="cuda")

    def launch(ap, lda, wp, ldw, b_, relu):
        out, ws = torch.full((M, Nn), SENTINEL, device="cuda"), nan_like((splits * M * Nn,))
        L.check(L.lib().mla_linear_splitk(ptr(ap), lda, ptr(wp), ldw, ptr(b_), ptr(out), Nn, M, Nn, kk, int(relu), splits, ptr(ws), ws.numel(),
                                          L.stream_ptr()))
        return out

    clean = check_gemm(lambda a_, w_, b_, relu: launch(a_, kk, w_, kk, b_, relu), K.gemm_reference, a, w, b, F32, "linear_splitk")
    for relu in (True, False):
        got = launch(padded(a, 2, 4, F32), kk + 4, padded(w, 1, 4, F32), kk + 4, b, relu)
        assert same_bits(got, clean[relu]), "e (relu=%d)" % relu


@pytest.mark.parametrize("which,M,Nn,kk", [("small", 70, 600, 128), ("small-wide", 5120, 600, 128), ("narrow", 70, 10, 600)])
def test_linear_small_and_narrow(ops, L, which, M, Nn, kk):
    """mla_linear_small (the head's 64-row kernel and its wide form) and mla_linear_narrow (N <= 16, through ops.linear) on grid
    operands: at most 600 products in units of 2^-6, so the f32 result is exact in any order. e: pitched NaN-padded a and w."""
    a, w, b = K.gemm_operands(M + kk, M, Nn, kk, device="cuda")
    lib = L.lib()

    def launch(ap, wp, b_, relu):
        assert not relu
        out = torch.full((M, Nn), SENTINEL, device="cuda")
        fn = lib.mla_linear_narrow if which == "narrow" else lib.mla_linear_small
        L.check(fn(ptr(ap), ap.stride(0), ptr(wp), wp.stride(0), ptr(b_), ptr(out), Nn, M, Nn, kk, L.stream_ptr()))
        return out

    clean = check_gemm(launch, K.gemm_reference, a, w, b, F32, "linear_" + which, relus=(False,))
    got = launch(padded(a, 2, 4, F32)[:M, :kk], padded(w, 1, 4, F32)[:Nn, :kk], b, False)
    assert same_bits(got, clean[False]), "e"
    if which == "narrow":       # ops.linear takes this route for such a shape
        assert same_bits(ops.linear(a, w, b), clean[False])


@pytest.mark.parametrize("case_id", ["64x128-seg64", "128x128-seg64"])
def test_linear_bf16x3(ops, case_id):
    """mla_linear_bf16x3 with f32 output on the sparse 2^-9 operands of test_linear_bf16x3_is_exact, against the three-product sum of
    the STORED planes (an Inf operand stores lo = inf - inf = NaN: the bf16x3 exception applies to pattern c only)."""
    M, Nn, kk, seg = K.X3_GEMM_CASES[case_id]
    c = K.x3_gemm_case(M + kk + seg, M, Nn, kk)

    def reference(a, w, b):
        (ah, al), (wh, wl) = K.planes(a), K.planes(w)
        ah, al, wh, wl = (t.double().cuda() for t in (ah, al, wh, wl))
        y = ah @ (wh + wl).t() + al @ wh.t() + b.double().cuda()
        return y, torch.nan_to_num(ah.abs() @ (wh.abs() + wl.abs()).t() + al.abs() @ wh.abs().t() + b.double().cuda().abs(), nan=0.0, posinf=0.0)

    def run(a, w, b, relu):
        return ops.linear_split(K.seg_planes_a(a.cpu(), seg).cuda(), K.seg_planes_w(w.cpu(), seg).cuda(), b.cuda(), seg, relu=relu, out_split=False)

    check_gemm(run, reference, c["a"], c["w"], c["b"], F32, "linear_bf16x3 " + case_id, x3=True)


# ----------------------------------------------------------------------------------------- 3. training twins ----

def emulate_codes(pre):
    """conv.hip's code_of on float64 pre-activations (NHWC): strict > in scan order, 4 where the running maximum is not > 0."""
    win = [pre[:, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]
    best, codes = win[0].clone(), torch.zeros(win[0].shape, dtype=torch.uint8)
    for k in (1, 2, 3):
        m = win[k] > best
        best, codes = torch.where(m, win[k], best), torch.where(m, torch.full_like(codes, k), codes)
    return torch.where(best > 0, codes, torch.full_like(codes, 4))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=name)
@pytest.mark.parametrize("layer", (2, 4, 6))
def test_conv3x3_train_and_codes(ops, layer, dtype):
    """mla_conv3x3_train (kept pre-pool activation + pooled output) and mla_conv3x3_train_codes (pooled output) at 5 images of the
    grid operands: the criterion of test_conv3x3_train_bf16_is_exact (round-to-nearest-even of the exact values). The window codes
    belong to the backward pass and are pinned in section 9."""
    case = K.conv_case(layer, "grid")
    n, cout = K.SMALL_N, case["w"].shape[0]

    def run(x, w, b):
        xs, wp = x.to(dtype).cuda()[:n], ops.repack_conv_weight(w.cuda(), dtype)
        a, p = ops.conv3x3_train(xs, wp, b.cuda(), cout)
        _, p2 = ops.conv3x3_train_codes(xs, wp, b.cuda(), cout)
        return a, p, p2

    clean = run(case["x"][:n], case["w"], case["b"])
    for pattern in N.CONV_PATTERNS:
        what = "conv3x3_train layer %d %s %s" % (layer, name(dtype), pattern)
        x, w, b, keep, channel = N.conv_inject(case, pattern, n)
        pooled_ref, pre = N.conv_reference(x[:n], w, b, True)
        got = run(x, w, b)
        for g, r, c, tag in zip(got, (F.relu(pre), pooled_ref, pooled_ref), clean, ("pre-pool", "pooled", "pooled (codes form)")):
            same_nonfinite(g, r, what + " " + tag, finite=N.exact(dtype))
            assert same_bits(g[keep], c[keep]), what + " " + tag
        if channel is not None:
            N.assert_channels(pooled_ref, channel, what)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=name)
def test_maxpool2x2(ops, dtype):
    """mla_maxpool2x2 / _bf16 on (3, 4, 6, 16) grid values: NaN in the four window positions of four windows, +inf, a window of -inf
    and one -inf among finite values, against F.max_pool2d in float64 (selection: equality)."""
    a = K.dyadic(torch.Generator().manual_seed(31), (3, 4, 6, 16))
    for pos, (y, x) in enumerate(((0, 0), (0, 3), (3, 0), (3, 5))):
        a[0, y, x, pos] = NAN
    a[1, 1, 1, 0], a[1, 0:2, 2:4, 1], a[1, 2, 4, 2] = INF, -INF, -INF
    ref = F.max_pool2d(a.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert int(torch.isnan(ref).sum()) == 4 and bool((ref == INF).any()) and bool((ref == -INF).any())
    got = ops.maxpool2x2(a.to(dtype).cuda())
    same_nonfinite(got, ref, "maxpool2x2 " + name(dtype), finite=N.exact(dtype))
    clean = ops.maxpool2x2(torch.nan_to_num(a, nan=0.0).to(dtype).cuda())
    assert same_bits(got[2], clean[2])


# ------------------------------------------------------------------------------------------- 4. ResNet trunk ----

import pin_leftover_cases as PL                                                      # noqa: E402
import resnet50_restated as RR                                                       # noqa: E402
import test_resnet_kernels_gpu as RK                                                 # noqa: E402

RN_DTYPES = [F32, BF16]


@pytest.mark.parametrize("dtype", RN_DTYPES, ids=name)
@pytest.mark.parametrize("shape", RK.CONV_SHAPES[:4], ids=str)
def test_rn_conv(ops, dtype, shape):
    """rn_conv 3x3 and 1x1 at stride 1 and 2 on non-square images (the first four shapes of test_conv_forward_is_exact: less than a
    tile, a tile plus a tail), raw and with scale / shift + residual + ReLU. Exact on the grid. e: the images are the head of an
    allocation with a NaN image behind them."""
    ks, stride, cin, cout, n, H, Wd = shape
    c = RK.conv_case(shape)
    pad = ks // 2

    def reference(x, w, scale, shift, res, full):
        y = RK.nhwc(F.conv2d(RK.nchw(x), w.double(), stride=stride, padding=pad))
        return F.relu(y * scale.double() + shift.double() + res.double()) if full else y

    def run(x, w, scale, shift, res, full):
        xs, wp = x.to(dtype).cuda()[:n], ops.rn_repack(w.cuda(), dtype)
        if not full:
            return ops.rn_conv(xs, wp, stride)
        return ops.rn_conv(xs, wp, stride, scale=scale.cuda(), shift=shift.cuda(), residual=res.to(dtype).cuda(), relu=True)

    base = (c["x"], c["w"], c["scale"], c["shift"], c["res_y"])
    clean = {full: run(*base, full) for full in (False, True)}
    for pattern in ("a", "b", "c", "d-weight", "d-scale", "d-shift", "res", "e"):
        x, w, scale, shift, res = (t.clone() for t in base)
        keep, channel = slice(0, 0), None
        if pattern == "a":
            x[0, H // 2, Wd // 2, cin // 2], keep = NAN, slice(1, n)
        elif pattern == "b":
            x[n - 1, H - 1, Wd - 1, cin - 1], keep = NAN, slice(0, n - 1)
        elif pattern == "c":
            x[0, 0, 0, 0], x[n - 1, H - 1, Wd - 1, 1] = INF, -INF
        elif pattern == "d-weight":
            channel = cout - 2
            w[channel, 3, pad, pad] = NAN
        elif pattern == "d-scale":
            channel = 5
            scale[channel] = NAN
        elif pattern == "d-shift":
            channel = 6
            shift[channel] = NAN
        elif pattern == "res":
            res[0, 0, 0, 7] = NAN
        else:
            x, keep = torch.cat([x, torch.full_like(x[:1], NAN)]), slice(0, n)
        for full in (False, True):
            if pattern in ("d-scale", "d-shift", "res") and not full:
                continue
            what = "rn_conv %s %s %s full=%d" % (shape, name(dtype), pattern, full)
            ref = reference(x[:n], w, scale, shift, res, full)
            got = run(x, w, scale, shift, res, full)
            same_nonfinite(got, ref, what, finite=N.exact(dtype))
            assert same_bits(got[keep], clean[full][keep]), what
            if channel is not None:
                N.assert_channels(ref, channel, what)
            if pattern == "res":
                assert int(torch.isnan(ref).sum()) == 1


@pytest.mark.parametrize("dtype", RN_DTYPES, ids=name)
def test_rn_bn_apply(ops, dtype):
    """rn_bn_apply on the dyadic operands of test_bn_apply_is_exact, 33 x 192: NaN and +-Inf in x, NaN in scale, shift and the
    residual, with and without residual and ReLU; the rows are the head of an allocation with NaN rows behind them."""
    rows, C = 33, 192
    gen = torch.Generator().manual_seed(70 + C)
    x, res = K.dyadic(gen, (rows, C)), K.dyadic(gen, (rows, C))
    scale, shift = RK.pow2_scale(gen, C), K.dyadic(gen, (C,))
    x[3, 17], x[32, 191], x[5, 8], x[6, 9] = NAN, NAN, INF, -INF
    scale[40], shift[41], res[7, 100] = NAN, NAN, NAN
    big = torch.cat([x, torch.full((4, C), NAN)]).to(dtype).cuda()
    for use_res, relu in ((False, False), (False, True), (True, True), (True, False)):
        ref = RK.apply_reference(x, scale, shift, res if use_res else None, False)
        ref = F.relu(ref) if relu else ref
        out = torch.full((rows, C), 9.0, dtype=dtype, device="cuda")
        ops.rn_bn_apply(big[:rows], scale.cuda(), shift.cuda(), residual=res.to(dtype).cuda() if use_res else None, relu=relu, out=out)
        same_nonfinite(out, ref, "rn_bn_apply %s res=%d relu=%d" % (name(dtype), use_res, relu), finite=N.exact(dtype))
        assert bool(torch.isnan(ref[:, 40]).all()) and bool(torch.isnan(ref[:, 41]).all()) and bool(torch.isinf(ref[5, 8]))
        assert float(ref[6, 9]) in ((0.0, INF) if relu else (-INF, INF))        # relu(-inf) = 0; the sign is the scale's


@pytest.mark.parametrize("dtype", RN_DTYPES, ids=name)
@pytest.mark.parametrize("H,Wd,C", [(2, 3, 8), (7, 5, 64), (9, 112, 8)])
def test_rn_maxpool(ops, dtype, H, Wd, C):
    """rn_maxpool (3, 2, 1) on the negative, -inf-strewn images of pool_case with NaN planted in a corner, in the last pixel and in
    the interior of image 0: equal to F.max_pool2d in float64, image 1 keeps the clean run's bits. Taps outside the image are
    skipped, never read as 0."""
    x = RK.pool_case(H, Wd, C)[0].clone()
    clean = ops.rn_maxpool(x.to(dtype).cuda())
    x[0, 0, 0, 0], x[0, H - 1, Wd - 1, C - 1], x[0, H // 2, Wd // 2, 3] = NAN, NAN, NAN
    ref = RK.nhwc(F.max_pool2d(RK.nchw(x), 3, 2, 1))
    got = ops.rn_maxpool(x.to(dtype).cuda())
    same_nonfinite(got, ref, "rn_maxpool %dx%dx%d %s" % (H, Wd, C, name(dtype)), finite=N.exact(dtype))
    assert bool(torch.isnan(ref).any()) and bool((x == -INF).any()) and same_bits(got[1], clean[1])


@pytest.mark.parametrize("dtype", RN_DTYPES, ids=name)
def test_rn_avgpool(ops, dtype):
    """rn_avgpool on (3, 3, 5, 104) grid values (hw = 15, C no multiple of 8 x 16): a NaN, a +inf, and +inf with -inf in one channel
    (NaN) -- the finite rest by test_avgpool_matches_float64's rule, one f32 division of an exact sum: 2^-24 |value|."""
    x = K.dyadic(torch.Generator().manual_seed(97), (3, 3, 5, 104))
    x[0, 1, 2, 5], x[1, 0, 0, 6], x[1, 2, 4, 7], x[1, 0, 1, 7] = NAN, INF, INF, -INF
    ref = x.double().sum(dim=(1, 2)) / 15
    assert bool(torch.isnan(ref[0, 5])) and float(ref[1, 6]) == INF and bool(torch.isnan(ref[1, 7])) and int((~torch.isfinite(ref)).sum()) == 3
    got = ops.rn_avgpool(x.to(dtype).cuda())
    same_nonfinite(got, ref, "rn_avgpool " + name(dtype), finite=N.bounded(RK.U * ref.abs(), "rn_avgpool " + name(dtype)))


@pytest.mark.parametrize("dtype", RN_DTYPES, ids=name)
def test_rn_bn_stats(ops, dtype):
    """rn_bn_stats on 97 x 192 (two ragged slices): a NaN poisons exactly its own channel -- scale, shift, mean, var and both running
    buffers -- and every other channel keeps the clean run's bits (which test_bn_stats_match_float64... bounds)."""
    RN = importlib.import_module(PKG + ".resnet")
    rows, C, ch = RK.SLICE_ROWS + 33, 192, 77
    x = RK.stats_input(rows, C, dtype, 41, "cuda")
    bad = x.clone()
    bad[rows - 2, ch] = NAN
    outs = []
    for t in (x, bad):
        bn = RK.bn_holder(RN, C, 50 + C)
        outs.append(list(ops.rn_bn_stats(t, bn, running=True, want_stats=True)) + [bn.running_mean, bn.running_var])
    other = torch.arange(C, device="cuda") != ch
    for clean, got in zip(*outs):
        assert bool(torch.isnan(got[ch])) and same_bits(got[other], clean[other]) and bool(torch.isfinite(clean).all())


@pytest.mark.parametrize("dtype", RN_DTYPES, ids=name)
@pytest.mark.parametrize("conf", ["repeat", "single"])
def test_rn_stem(ops, dtype, conf):
    """rn_stem on two 224 x 224 planes against float64 conv2d of the normalised channels (the per-element derived bound of
    test_rn_stem_every_element_within_its_derived_bound: 55 roundings on sum|terms|, plus half a bf16 ulp; it is below the 1e-4 / 1e-2
    of the largest value that test_stem_borders grants, which is asserted). A NaN pixel in the interior and one in a corner of plane
    0 (taps outside the image are skipped: the corner NaN reaches only the outputs whose window holds it); plane 1 keeps the clean
    run's bits. A NaN in a CORNER tap of one filter makes that whole channel NaN, border pixels included: nn.Conv2d multiplies its
    zero padding with it."""
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 224, 224, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.05
    tol = 1e-4 if dtype == F32 else 1e-2

    def check(x, w, what):
        acc, terms = PL.stem_reference(x, w, conf)
        ref, bound = PL.stem_bound(acc, terms, None, None, False, dtype)
        got = ops.rn_stem(x.cuda(), conf == "single", w.cuda(), dtype)
        top = float(ref[torch.isfinite(ref)].abs().max())
        assert float(bound[torch.isfinite(bound)].max()) <= tol * top
        same_nonfinite(got, ref, what, finite=N.bounded(bound, what))
        return got, ref

    clean, _ = check(x, w, "rn_stem clean")
    bad = x.clone()
    bad[0, 100, 101], bad[0, 0, 0], bad[0, 223, 223] = NAN, NAN, NAN
    got, ref = check(bad, w, "rn_stem %s %s NaN pixels" % (conf, name(dtype)))
    assert int(torch.isnan(ref[0, :, :, 0]).sum()) == 3 * 4 + 4 + 4 and not bool(torch.isnan(ref[1]).any()) and same_bits(got[1], clean[1])
    wbad = w.clone()
    wbad[5, 1 if conf == "single" else 0, 0, 0] = NAN
    _, ref = check(x, wbad, "rn_stem %s %s NaN corner tap" % (conf, name(dtype)))
    N.assert_channels(ref, 5, "rn_stem NaN tap")


# --------------------------------------------------------------------------------------------------- 5. head ----

import test_train_kernels_gpu as TK                                                  # noqa: E402
import test_wide_head_gpu as WH                                                      # noqa: E402


def same_as_clean_but(got, clean, ref, what, touched=None):
    """For kernels whose finite criterion is a derived or recorded tolerance: NaN and +-inf sit exactly where the float64 reference has
    them, and every other element keeps the BITS of the clean run of the same operands, which the sibling finite test holds to that
    tolerance. `touched`: elements the injection changes to another finite value (relu(-inf) = 0, sigmoid(+-inf) = 1, 0): they must
    equal the reference exactly."""
    fin = same_nonfinite(got, ref, what).to(got.device)
    if touched is not None:
        touched = touched.to(got.device) & fin
        assert bool(torch.equal(got[touched].double(), ref.to(got.device)[touched])), what + ": touched finite elements"
        fin = fin & ~touched
    assert same_bits(got[fin], clean[fin]), what + ": an element the injection does not reach changed"


def head_bn_forward(x, mean, var, gamma, beta, mode, period, act, keep, drop_scale):
    """float64 y = act((x - mean) / sqrt(var + eps) gamma + beta) [* keep * drop_scale], as F.dropout multiplies."""
    xc = TK._bn_channels(x.double(), mode, period)
    m, v, g, b = (t.double().reshape(1, -1, 1) for t in (mean, var, gamma, beta))
    y = (xc - m) / torch.sqrt(v + TK.EPS) * g + b
    y = torch.relu(y) if act == 1 else torch.sigmoid(y) if act == 2 else y
    y = y.reshape(x.shape)
    return y if keep is None else y * keep.reshape(x.shape).double() * drop_scale


@pytest.mark.parametrize("mode,period,rows,cols", [(0, 10, 70, 600), (1, 0, 37, 64)])
def test_head_bn_stats_and_apply(ops, W, mode, period, rows, cols):
    """mla_bn_stats and mla_bn_apply in both layouts (channel = row % period, channel = column), acts 0 / 1 / 2, with and without a
    keep mask. Statistics: the clean run within the per-channel derived bounds of tests/test_pin_leftovers_gpu.py; a NaN poisons its
    own channel's mean and variance and no other (the others keep the clean run's bits). Apply, with the clean statistics: a NaN at
    a DROPPED element stays NaN (F.dropout multiplies: NaN * 0), +inf gives +inf / +inf / 1, -inf gives -inf / 0 / 0, a dropped
    +inf gives NaN; a NaN in gamma, beta, mean or var makes exactly that channel NaN."""
    ch = period if mode == 0 else cols
    x, _, gamma, beta, keep, drop_scale = TK._bn_inputs(W, 440 + cols, rows, cols, ch, 1)
    keep2 = keep.reshape(rows, cols)
    dropped, kept = (keep2 == 0).nonzero(), (keep2 != 0).nonzero()
    (r0, c0), (r1, c1), (r2, c2), (r3, c3) = (tuple(int(v) for v in t) for t in (dropped[3], kept[5], kept[40], dropped[50]))
    channel_of = lambda r, c: r % period if mode == 0 else c                                      # noqa: E731
    bad = x.clone()
    bad[r0, c0], bad[r1, c1], bad[r2, c2], bad[r3, c3] = NAN, INF, -INF, INF
    mean, var = ops.bn_stats(x.cuda(), mode, period)
    stats = PL.stats_reference(x, torch.zeros(ch), torch.ones(ch), mode, period)       # the clean run: test_pin_leftovers_gpu's criterion
    for got, k in ((mean, "mean"), (var, "var")):
        WH.within(got, stats[k], stats["b_" + k], "bn_stats mode %d clean %s" % (mode, k))
    mean_b, var_b = ops.bn_stats(torch.where(torch.isinf(bad), x, bad).cuda(), mode, period)
    other = torch.arange(ch, device="cuda") != channel_of(r0, c0)
    for clean, got in ((mean, mean_b), (var, var_b)):
        assert bool(torch.isnan(got[~other]).all()) and same_bits(got[other], clean[other]) and bool(torch.isfinite(clean).all())
    touched = torch.zeros(rows, cols, dtype=torch.bool)
    touched[r1, c1] = touched[r2, c2] = touched[r3, c3] = True          # finite after relu (0) or the sigmoid (0, 1): exact values
    for act in (0, 1, 2):
        for mask in (None, keep):
            what = "bn_apply mode %d act %d mask %s" % (mode, act, mask is not None)
            args = (mode, period, mean, var, gamma.cuda(), beta.cuda())
            kw = dict(act=act, keep_mask=None if mask is None else mask.cuda(), drop_scale=drop_scale if mask is not None else 1.0)
            clean = ops.bn_apply(x.cuda(), *args, **kw)
            ref = head_bn_forward(bad, mean.cpu(), var.cpu(), gamma, beta, mode, period, act, mask, kw["drop_scale"])
            same_as_clean_but(ops.bn_apply(bad.cuda(), *args, **kw), clean, ref, what, touched=touched if act else None)
    for which in range(4):
        params = [mean.cpu().clone(), var.cpu().clone(), gamma.clone(), beta.clone()]
        params[which][ch // 2] = NAN
        ref = head_bn_forward(x, *params, mode, period, 1, keep, drop_scale)
        N.assert_channels(TK._bn_channels(ref, mode, period), ch // 2, "bn_apply parameter %d" % which, axis=1)
        got = ops.bn_apply(x.cuda(), mode, period, *[p.cuda() for p in params], act=1, keep_mask=keep.cuda(), drop_scale=drop_scale)
        clean = ops.bn_apply(x.cuda(), mode, period, mean, var, gamma.cuda(), beta.cuda(), act=1, keep_mask=keep.cuda(), drop_scale=drop_scale)
        same_as_clean_but(got, clean, ref, "bn_apply NaN in parameter %d" % which)


@pytest.mark.parametrize("T,Kc,bags", [(10, 10, 17), (7, 16, 33), (10, 527, 5), (17, 10, 3)])
def test_attention_pool(ops, W, T, Kc, bags):
    """mla_attention_pool, the register kernel (K <= 16, T <= 16) and the wide one: a NaN in z[bag, t, k] makes the reference's
    entries of y[bag, :] NaN -- all of them: softmax over k spreads it along the row, the sum over t along the columns -- and no
    other bag changes a bit. y is a column slice between sentinels."""
    z, nv, nf, _ = WH._attention_inputs(W, T, Kc, bags, 5.0)
    bag = bags // 2
    bad = z.clone()
    bad[bag, T - 1, Kc // 2] = NAN
    ref = TK._attention_reference(bad, nv, nf, T)[4].detach()
    assert bool(torch.isnan(ref[bag]).all()) and int(torch.isnan(ref).sum()) == Kc
    outs = []
    for t in (z, bad):
        ybuf = torch.full((bags, Kc + 5), -7.25, device="cuda")
        ops.attention_pool(t.reshape(bags * T, Kc).cuda(), bags, T, Kc, [p.cuda() for p in nv], [p.cuda() for p in nf], ybuf[:, 2:2 + Kc])
        outs.append(ybuf)
    clean, got = outs
    same_as_clean_but(got[:, 2:2 + Kc], clean[:, 2:2 + Kc], ref, "attention_pool T %d K %d" % (T, Kc))
    assert bool((got[:, :2] == -7.25).all()) and bool((got[:, 2 + Kc:] == -7.25).all())


def test_gather_bags_copies_bits(ops):
    """mla_gather_bags: a copy. NaN and +-inf rows arrive bit for bit; a NaN row no window holds appears nowhere."""
    T = 10
    emb = torch.randn((31, 128), generator=torch.Generator().manual_seed(3))
    emb[5, 7], emb[12, 0], emb[12, 127], emb[30, :] = NAN, INF, -INF, NAN
    first = np.array([7, 0, 3, 20, 3], dtype=np.int64)
    idx = (torch.from_numpy(first)[:, None] + torch.arange(T)).reshape(-1)
    got = ops.gather_bags(emb.cuda(), first, T)
    assert same_bits(got.cpu(), emb[idx]) and int(torch.isnan(got).sum()) == 3 and int(torch.isinf(got).sum()) == 6     # row 5: 3 windows


# ------------------------------------------------------------------------------------- 6. loss and optimizer ----

def test_cross_entropy_with_nan_logits(ops, W):
    """mla_cross_entropy, 257 rows x 10: a NaN logit in the first column of one row and in a later column of another. The loss is NaN
    as F.cross_entropy's, hits[1] == 0 and raise_on_bad_labels does not raise (a NaN loss is not a bad label), the two dscores rows
    are NaN as autograd's, every other row keeps the clean run's bits, and the hit count lies between the count over the finite rows
    and that count plus the two NaN rows."""
    rows, Kc = 257, 10
    x, labels = TK._ce_inputs(W, rows, Kc, 4.0, 600 + rows + Kc)
    inv_total = 1.0 / rows
    _, d_clean, hits_clean = ops.cross_entropy(TK.strided(x, 2, 1), labels.cuda(), inv_total)
    bad = x.clone()
    bad[100, 0], bad[256, 7] = NAN, NAN
    x64 = bad.double().requires_grad_(True)
    ref = F.cross_entropy(x64, labels, reduction="sum") * inv_total
    ref.backward()
    assert math.isnan(float(ref.detach()))
    loss, d, hits = ops.cross_entropy(TK.strided(bad, 2, 1), labels.cuda(), inv_total)
    assert math.isnan(float(loss)) and int(hits[1]) == 0
    finite_rows = torch.ones(rows, dtype=torch.bool)
    finite_rows[[100, 256]] = False
    base = int((torch.argmax(x, dim=1) == labels)[finite_rows].sum())
    assert base <= ops.raise_on_bad_labels(hits) <= base + 2
    same_as_clean_but(d, d_clean, x64.grad, "cross_entropy dscores")
    assert bool(torch.isnan(x64.grad[100]).all()) and bool(torch.isnan(x64.grad[256]).all()) and int(torch.isnan(x64.grad).sum()) == 2 * Kc
    loss2, _, hits2 = ops.cross_entropy(TK.strided(bad, 2, 1), labels.cuda(), inv_total, want_grad=False)
    assert math.isnan(float(loss2)) and torch.equal(hits2, hits)


@pytest.mark.parametrize("dev_form", [False, True], ids=["adam_step", "adam_step_dev"])
def test_adam_with_a_nan_gradient(ops, W, dev_form):
    """mla_adam_step / mla_adam_step_dev, 257 elements, three steps with a NaN gradient element in the second: that parameter and
    both its moments are NaN from then on, as float64 torch.optim.Adam's, and every other element keeps the clean run's bits."""
    n, at = 257, 130
    p0 = TK.rnd(W, 700, n, (n,), -0.05, 0.05)
    state = {k: [p0.cuda().clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")] for k in ("clean", "bad")}
    p64 = p0.double().requires_grad_(True)
    opt = torch.optim.Adam([p64], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    scal, ctr = torch.zeros(2, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    for step in (1, 2, 3):
        g = TK.rnd(W, 700 + step, n, (n,), -1.0, 1.0)
        gb = g.clone()
        if step == 2:
            gb[at] = NAN
        for k, grad in (("clean", g), ("bad", gb)):
            p, m, v = state[k]
            if dev_form:
                ops.adam_prepare(scal, 1e-3, 0.9, 0.999, step)
                ops.adam_step_dev(p, grad.cuda(), m, v, 0.9, 0.999, 1e-8, scal, ctr)
            else:
                ops.adam_step(p, grad.cuda(), m, v, 1e-3, 0.9, 0.999, 1e-8, step)
        p64.grad = gb.double()
        opt.step()
    st = opt.state[p64]
    for got, clean, ref in zip(state["bad"], state["clean"], (p64.detach(), st["exp_avg"], st["exp_avg_sq"])):
        assert bool(torch.isnan(ref[at])) and int(torch.isnan(ref).sum()) == 1
        same_as_clean_but(got, clean, ref, "adam")


def test_axpy_col_sum_and_transpose_padded(ops, W):
    """mla_axpy: y += a x keeps a NaN / Inf of x or y in its own element. mla_col_sum: a NaN poisons its own column's sum only.
    transpose_padded (f32 and bf16): NaN and Inf move with their element, and the zero padding behind R stays exactly 0."""
    n = 257
    x, y = TK.rnd(W, 710, n, (n,), -2.0, 2.0), TK.rnd(W, 711, n, (n,), -2.0, 2.0)
    clean = ops.axpy(0.3, x.cuda(), y.cuda())
    xb, yb = x.clone(), y.clone()
    xb[3], xb[200], yb[256], yb[100] = NAN, INF, NAN, -INF
    ref = yb.double() + float(np.float32(0.3)) * xb.double()
    same_as_clean_but(ops.axpy(0.3, xb.cuda(), yb.cuda()), clean, ref, "axpy")
    for dtype, rows, cols in ((F32, 70, 600), (F32, 37, 10), (BF16, 70, 600)):
        a = K.dyadic(torch.Generator().manual_seed(rows), (rows, cols)).to(dtype)
        out_c, out_b = torch.full((cols,), 9.0, device="cuda"), torch.full((cols,), 9.0, device="cuda")
        ops.col_sum(a.cuda(), out_c)
        b = a.clone()
        b[rows - 1, 5], b[0, cols - 1] = NAN, INF
        ops.col_sum(b.cuda(), out_b)
        same_as_clean_but(out_b, out_c, b.double().sum(dim=0), "col_sum %s %dx%d" % (name(dtype), rows, cols))
        assert torch.equal(out_c.cpu().double(), a.double().sum(dim=0))
    for dtype, per in ((F32, 4), (BF16, 8)):
        R_, C_ = 77, 50
        t = K.dyadic(torch.Generator().manual_seed(9), (R_, C_)).to(dtype)
        t[0, 0], t[76, 49], t[40, 3], t[76, 0] = NAN, NAN, INF, -INF
        got = ops.transpose_padded(t.cuda()).cpu()
        ld = (R_ + per - 1) // per * per
        assert tuple(got.shape) == (C_, ld) and same_bits(got[:, :R_].contiguous(), t.t().contiguous())
        assert not bool(N._bits(got[:, R_:].contiguous()).any()), "the padding is not exactly +0"


# ---------------------------------------------------------------------------------------------- 7. postprocessor ----

def test_postprocess_with_a_nan_embedding(W):
    """mla_postprocess (vggish.Postprocessor): a NaN embedding element makes its whole row NaN -- every PCA component sums over it, and
    torch.clamp keeps NaN -- exactly as oracle.model.postprocess; the other rows keep the clean run's bits. A +-inf element gives
    inf * e: +inf -> 255, -inf -> 0 after the clamp, NaN where the eigenvector entry is 0 (none here)."""
    from oracle import model as omodel
    vg = importlib.import_module(PKG + ".torchvggish.vggish")
    ev = torch.as_tensor(W.uniform(2, W.stream_id("pca_eigen_vectors"), 128 * 128).reshape(128, 128) * 0.5).float()
    mu = torch.as_tensor(W.uniform(2, W.stream_id("pca_means"), 128).reshape(128, 1) * 0.5).float()
    pp = vg.Postprocessor()
    pp.load_state_dict({"pca_eigen_vectors": ev, "pca_means": mu})
    pp = pp.cuda()
    emb = torch.as_tensor(W.uniform(2, 77, 5 * 128, lo=-1.0, hi=1.0).reshape(5, 128)).float()
    bad = emb.clone()
    bad[1, 64], bad[3, 5] = NAN, INF
    clean, got = pp(emb.cuda()), pp(bad.cuda())
    ref = omodel.postprocess(ev.double(), mu.double(), bad.double())
    assert bool(torch.isnan(ref[1]).all()) and int(torch.isnan(ref).sum()) == 128 and set(ref[3].tolist()) == {0.0, 255.0}
    touched = torch.zeros(5, 128, dtype=torch.bool)
    touched[3] = True
    same_as_clean_but(got, clean, ref, "postprocess", touched=touched)


# -------------------------------------------------------------------------------------------------- 8. front-ends ----

import functools                                                                     # noqa: E402

import librosa_htk_restated as H                                                     # noqa: E402
import librosa_restated as R                                                         # noqa: E402
import test_clips_cpu as C                                                           # noqa: E402
import test_logmel_bags_cpu as B                                                     # noqa: E402
from oracle import dataset_frames as ods                                             # noqa: E402
from oracle import frontend as ofe                                                   # noqa: E402
from oracle import model as omodel                                                   # noqa: E402
from oracle import resample as oresample                                             # noqa: E402


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def test_waveforms_to_examples_with_a_nan_sample(fe, W):
    """mla_logmel_examples, two waveforms of three examples: NaN where oracle.frontend.batch_examples (float64) has it -- every band of
    the frames whose window holds the sample -- and everything else keeps the clean run's bits."""
    wav = W.waveform(5, 15600 + 2 * 15360, 2).astype(np.float32)
    bad = N.nan_sample(wav, (0, 23456))
    ref = torch.from_numpy(np.asarray(ofe.batch_examples(bad.astype(np.float64))))
    for out_dtype in (F32, BF16):
        clean, got = fe.waveforms_to_examples(dev(wav), out_dtype), fe.waveforms_to_examples(dev(bad), out_dtype)
        same_as_clean_but(got, clean, ref.reshape(got.shape), "waveforms_to_examples " + name(out_dtype))
    assert 0 < int(torch.isnan(ref).sum()) < ref.numel() // 6 and int(torch.isnan(ref).sum()) % 64 == 0


@pytest.mark.parametrize("n_frames,stride", [(10, 32), (4, 96)])
def test_logmel_bags_with_a_nan_sample(fe, n_frames, stride):
    """mla_logmel_bags on the ragged rows of test_logmel_bags_cpu: a NaN sample in the two-example row, against the float64 chain
    split(create_spec_native(x)); the other rows keep the clean run's bits."""
    rows, counts = B.rows_and_counts()
    i = B.LENGTHS.index(30960)
    bad = N.nan_sample(rows, (i, 20000))
    clean, got = fe.logmel_bags(dev(rows), counts, n_frames, stride), fe.logmel_bags(dev(bad), counts, n_frames, stride)
    ref = torch.from_numpy(np.stack([np.asarray(ods.split(ods.create_spec_native(bad[j, :min(n, B.ROW)].astype(np.float64)), 10, 96, 64, stride == 32))
                                     if j == i else np.zeros((n_frames, 64, 96)) for j, n in enumerate(B.LENGTHS)]))
    assert bool(torch.isnan(ref[i]).any()) and not bool(torch.isnan(ref[i]).all())
    same_as_clean_but(got[:, :, 0], clean[:, :, 0], ref, "logmel_bags (%d, %d)" % (n_frames, stride))


def test_logmel_timeline_with_a_nan_sample(fe):
    """mla_logmel_timeline, two recordings at a hop of 3 slots: with a NaN sample in recording 0 every whole window still is, bit
    for bit and NaN included, the logmel_bags bag of its crop (the timeline test's criterion; logmel_bags is held to the float64
    chain above), some windows hold the NaN and some do not, and recording 1 keeps the clean run's bits."""
    q, n0, n1 = 3, 128000, 61680
    pcm = np.zeros((2, n0), dtype=np.float32)
    pcm[0], pcm[1, :n1] = B.noise(20, n0), B.noise(21, n1)
    bad = N.nan_sample(pcm, (0, 70000))
    (clean, first, rec), (got, _, _) = fe.logmel_timeline(dev(pcm), [n0, n1], q), fe.logmel_timeline(dev(bad), [n0, n1], q)
    nan_windows = 0
    for w in np.nonzero(rec == 0)[0]:
        j = int(w)
        crop = bad[0, 5120 * q * j:][:61680]
        if len(crop) < 61680:
            continue
        bag = fe.logmel_bags(dev(crop[None]), [4])[0, :, 0]
        assert same_bits(got[first[w]:first[w] + 10], bag), w
        nan_windows += int(torch.isnan(bag).any())
    assert 0 < nan_windows < int((rec == 0).sum())
    lo = int(first[np.nonzero(rec == 1)[0][0]])
    assert same_bits(got[lo:], clean[lo:]) and not bool(torch.isnan(got[lo:]).any())


def check_db(D, clean, ref_power, what):
    """(clips, bands, frames) dB against the float64 powers: NaN in every band of the frames the sample reaches, clean bits elsewhere."""
    ref = torch.from_numpy(10.0 * np.log10(np.maximum(R.AMIN, ref_power)))
    assert 0 < int(torch.isnan(ref).sum()) < ref.numel() // 2
    same_as_clean_but(D, clean, ref, what)


def test_melspec_with_a_nan_sample(fe):
    """melspec_db_unclipped + melspec_images (centre padding, the ResNet branch): a NaN sample in clip 0 of three. D is NaN in the
    frames that read it (librosa_restated: np.maximum(amin, .) keeps NaN). The clip maximum is then NaN, so power_to_db's
    np.maximum(D, D.max() - top_db) makes EVERY element of that clip's images NaN; the other clips keep the clean run's bits."""
    n, hop, n_mels = 5000, 98, 224
    waves = np.stack([R.waveform(nm, n) for nm in ("noise", "chirp", "burst")])
    bad = N.nan_sample(waves, (0, 2500))
    (Dc, wc), (Db, wb) = fe.melspec_db_unclipped(dev(waves), 22050, n_mels, hop), fe.melspec_db_unclipped(dev(bad), 22050, n_mels, hop)
    check_db(Db, Dc, np.stack([R.mel_power(w, 22050, n_mels, hop) for w in bad]), "melspec_db_unclipped")
    args = (n, hop, 80.0, 3, 20, 16)                                   # 52 frames: 2 * 16 + 20
    clean, got = fe.melspec_images(Dc, wc, *args), fe.melspec_images(Db, wb, *args)
    ref = torch.from_numpy(np.stack([R.split(R.melspectrogram_db(w, 22050, n_mels, hop), 3, 20, True) if i else np.full((3, n_mels, 20), np.nan)
                                     for i, w in enumerate(bad)]))
    assert np.isnan(R.melspectrogram_db(bad[0], 22050, n_mels, hop)).all() and R.split_step(52, 3, 20, True) == 16
    same_as_clean_but(got[:, :, 0], clean[:, :, 0], ref, "melspec_images")
    assert bool(torch.isnan(got[0]).all()) and not bool(torch.isnan(got[1:]).any())


@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=name)
def test_melspec_librosa_with_a_nan_sample(fe, out_dtype):
    """melspec_db_unclipped_librosa + melspec_bags (no padding, HTK basis, the VGGish branch's librosa path): the same, 20 frames."""
    n = 5088
    waves = np.stack([H.clip_waveform(nm, n) for nm in ("noise", "chirp")])
    bad = N.nan_sample(waves, (0, 3000))
    kw = dict(fmin=H.FMIN, fmax=H.FMAX, htk=True)
    (Dc, wc), (Db, wb) = (fe.melspec_db_unclipped_librosa(dev(w), H.SR, H.N_MELS, H.HOP, **kw) for w in (waves, bad))
    check_db(Db, Dc, np.stack([H.mel_power(w) for w in bad]), "melspec_db_unclipped_librosa")
    args = (n, H.HOP, 80.0, 2, 12, 8)                                  # 20 frames: 8 + 12
    clean, got = fe.melspec_bags(Dc, wc, *args, out_dtype=out_dtype), fe.melspec_bags(Db, wb, *args, out_dtype=out_dtype)
    assert np.isnan(H.melspectrogram_db(bad[0])).all()
    assert bool(torch.isnan(got[0]).all()) and same_bits(got[1], clean[1]) and not bool(torch.isnan(got[1]).any())


def test_prepare_clips_and_resample_with_a_nan_sample(fe):
    """mla_clips_prepare on four float recordings (48 kHz mono, 44.1 kHz stereo, 8 kHz upsampled, a 22.05 kHz copy) with a NaN in one
    sample of each of the first two (one channel of the stereo frame), and fe.resample on the first alone: NaN exactly where
    oracle/resample.py's float64 filter reaches the sample, the other outputs and recordings keep the clean run's bits."""
    idx = (1, 0, 2, 8)
    recs = [C.make_recording(i, False) for i in idx]
    rates = [C.ALL_CASES[i][0] for i in idx]
    bad = [r.copy() for r in recs]
    bad[0][2500] = np.nan
    bad[1][3000, 1] = np.nan
    outs = []
    for rr in (recs, bad):
        packed, offsets, frames, channels = C.pack(rr)
        outs.append(fe.prepare_clips(dev(packed), offsets, frames, channels, rates, C.SR_OUT, 2048))
    ref = torch.from_numpy(np.stack([C.cut_and_fill(C.resampled_f64(r, sr), 2048) for r, sr in zip(bad, rates)]))
    assert all(0 < int(torch.isnan(ref[i]).sum()) < 2048 for i in (0, 1)) and not bool(torch.isnan(ref[2:]).any())
    same_as_clean_but(outs[1], outs[0], ref, "prepare_clips")
    clean, got = fe.resample(dev(recs[0]), rates[0], C.SR_OUT), fe.resample(dev(bad[0]), rates[0], C.SR_OUT)
    same_as_clean_but(got, clean, torch.from_numpy(oresample.resample(bad[0].astype(np.float64), rates[0], C.SR_OUT)), "resample")


# -------------------------------------------------------------------------------------------------- 9. end to end ----

VG_CONF = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False, cnn_trainable=False,
               first_cnn_layer_trainable=False, in_channels=1)
BAGS = 4
CONV_KEY = "cnn.cnn_model.features.6.weight"


@functools.lru_cache(maxsize=None)
def vggish_case(kind):
    """Four bags of 10 s PCM and the seeded weights, with a NaN sample in bag 0 ('sample') or in one conv3 weight ('weight'), and the
    oracle's scores (float32 CPU restatement of the reference) -- computed once for the three precisions."""
    Wm = importlib.import_module(PKG + ".weights")
    sd = dict(Wm.make_state_dict(6, Wm.ensemble_shapes((2, 1), False)))
    wav = Wm.waveform(5, 160000, BAGS).astype(np.float32)
    if kind == "sample":
        wav[0, 77777] = np.nan
    elif kind == "weight":
        sd[CONV_KEY] = np.array(sd[CONV_KEY], copy=True)
        sd[CONV_KEY][3, 7, 1, 1] = np.nan
    if kind == "clean":
        return sd, wav, None
    with torch.no_grad():
        ref = omodel.ensemble_forward(omodel.to_torch(sd), torch.as_tensor(ofe.batch_examples(wav.astype(np.float64))).float())
    return sd, wav, ref


def vggish_ensemble(sd, prec):
    M = importlib.import_module(PKG + ".model")
    ens = M.Ensemble("repeat", dict(VG_CONF), [2, 1], torch.device("cuda"))
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return ens.cuda().eval().set_precision(prec)


@pytest.mark.parametrize("prec", ["f32", "bf16", "bf16x3"])
def test_ensemble_vggish_eval_forward(prec):
    """Ensemble.forward_waveforms, VGGish trunk, 4 bags: with a NaN sample in bag 0 isnan(scores) is the oracle's (bag 0, every
    class) and bags 1..3 keep the clean forward's bits; with a NaN in one conv weight every score is NaN, as the oracle's."""
    sd, wav, _ = vggish_case("clean")
    ens = vggish_ensemble(sd, prec)
    with torch.no_grad():
        clean = ens.forward_waveforms(dev(wav))
        assert bool(torch.isfinite(clean).all())
        _, bad, ref = vggish_case("sample")
        got = ens.forward_waveforms(dev(bad))
        assert bool(torch.isnan(ref[0]).all()) and not bool(torch.isnan(ref[1:]).any())
        assert torch.equal(torch.isnan(got).cpu(), torch.isnan(ref)) and same_bits(got[1:], clean[1:])
        sdw, _, ref = vggish_case("weight")
        got = vggish_ensemble(sdw, prec).forward_waveforms(dev(wav))
        assert bool(torch.isnan(ref).all()) and torch.equal(torch.isnan(got).cpu(), torch.isnan(ref))


@functools.lru_cache(maxsize=None)
def resnet_case(kind):
    import test_resnet_gpu as TG
    sd = dict(TG.state_dict())
    x = TG.images(31, BAGS).float()
    if kind == "sample":
        x[0, 4, 0, 100, 101] = NAN
    elif kind == "weight":
        key = [k for k, v in sd.items() if k.startswith("cnn.") and np.ndim(v) == 4 and np.shape(v)[-1] == 3][3]
        sd[key] = np.array(sd[key], copy=True)
        sd[key][2, 5, 1, 1] = np.nan
    if kind == "clean":
        return sd, x, None
    net = RR.CNN(True).float()
    net.load_state_dict({k[4:]: torch.as_tensor(v) for k, v in sd.items() if k.startswith("cnn.")})
    with torch.no_grad():
        feat = net.eval()(RR.normalize_input(x, "repeat"))
        ref = omodel.mla_forward(omodel.to_torch(sd), feat.reshape(BAGS, 10, 2048))
    return sd, x, ref


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_ensemble_resnet_eval_forward(prec):
    """Ensemble eval forward, ResNet trunk, 4 bags of ten 224 x 224 images: a NaN pixel in bag 0, and separately a NaN in one 3 x 3
    conv weight, against the restated ResNet-50 + the oracle's head (float32 on the CPU: only the NaN positions are compared)."""
    M = importlib.import_module(PKG + ".model")
    import test_resnet_gpu as TG

    def ensemble(sd):
        ens = M.Ensemble("repeat", dict(TG.CONF), [2, 1], torch.device("cuda"), precision=prec)
        ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        return ens.cuda().eval()

    sd, x, _ = resnet_case("clean")
    ens = ensemble(sd)
    with torch.no_grad():
        clean = ens(x.cuda())
        assert bool(torch.isfinite(clean).all())
        _, bad, ref = resnet_case("sample")
        got = ens(bad.cuda())
        assert bool(torch.isnan(ref[0]).all()) and not bool(torch.isnan(ref[1:]).any())
        assert torch.equal(torch.isnan(got).cpu(), torch.isnan(ref)) and same_bits(got[1:], clean[1:])
        sdw, _, ref = resnet_case("weight")
        got = ensemble(sdw)(x.cuda())
        assert bool(torch.isnan(ref).all()) and torch.equal(torch.isnan(got).cpu(), torch.isnan(ref))


@functools.lru_cache(maxsize=None)
def oracle_train_loss():
    """The oracle's train-mode loss on the step-2 batch below (NaN input element): forward only, any masks."""
    import make_golden as mk
    Wm = importlib.import_module(PKG + ".weights")
    x, y = mk.synth_bags(302, BAGS)
    x[0, 3, 0, 40, 30] = NAN
    sd = omodel.to_torch(Wm.make_state_dict(7, Wm.ensemble_shapes((2, 1), False)))
    with torch.no_grad():
        out = omodel.ensemble_forward(sd, x.float(), train=True, masks=mk.make_masks(1, (2, 1), BAGS))
    return float(F.cross_entropy(out, y))


@pytest.mark.parametrize("precision,finetune", [("f32", False), ("bf16", False), ("f32", True), ("bf16", True)])
def test_train_step_with_a_nan_input(mk, W, precision, finetune):
    """TrainStep, frozen and fine-tune, 4 bags: a clean step, then a step with one NaN input element. Train-mode BatchNorm spreads it
    over the batch: the loss is NaN, as the oracle's, no label is reported bad, and the graph replay gives the eager step's bits --
    loss, hit counts, every parameter and both Adam moments, compared as integers (NaN != NaN as floats)."""
    from test_train_graph_gpu import make
    assert math.isnan(oracle_train_loss())
    runs = []
    ords = None
    for graph in (False, True):
        _, step, ords = make(mk, W, precision, finetune, graph=graph, ordinals=ords)
        out = []
        for s in (301, 302):
            x, y = mk.synth_bags(s, BAGS)
            if s == 302:
                x[0, 3, 0, 40, 30] = NAN
            loss, hits = step(x.cuda(), y.cuda())
            out.append((loss.clone(), hits.clone()))
        runs.append((step, out))
    (step_e, out_e), (step_g, out_g) = runs
    assert step_e._graph is None and step_g._graph is not None
    assert math.isfinite(float(out_e[0][0])) and math.isnan(float(out_e[1][0])) and int(out_e[1][1][1]) == 0
    importlib.import_module(PKG + ".ops").raise_on_bad_labels(out_e[1][1])
    for (le, he), (lg, hg) in zip(out_e, out_g):
        assert same_bits(le, lg) and torch.equal(he, hg)
    for a, b in ((step_e.flat_p, step_g.flat_p), (step_e.flat_m, step_g.flat_m), (step_e.flat_v, step_g.flat_v)):
        assert same_bits(a, b) and bool(torch.isnan(a).any())


# ------------------------------------------------------------------- 10. the backward masks, pinned as they are ----
# torch's threshold_backward passes the gradient where the saved activation is NaN (NaN <= 0 is false); these kernels test
# `a > 0` and pass 0, and the pooling routes never choose a NaN that is not the window's first tap. Left as they are on purpose
# (DESIGN.md section 5): once the forward propagates, the NaN reaches the loss. A change here should be deliberate.

def test_pinned_relu_pool_bwd_treats_nan_as_not_positive(ops):
    """mla_relu_pool_bwd (f32) and mla_relu_pool_bwd_bf16. Un-pooled: a NaN activation gets gradient 0, i.e. the bits of the run with
    0 in its place. Pooled: a NaN in a later window position is never the maximum -- the bits of the run with -inf in its place;
    a NaN in the FIRST position is kept as the running maximum, nothing is > 0, and the whole window gets 0."""
    for dtype in (F32, BF16):
        gen = torch.Generator().manual_seed(77)
        a = K.dyadic(gen, (2, 4, 6, 16)).clamp_min(0).to(dtype)
        d, dp = K.dyadic(gen, (2, 4, 6, 16)).to(dtype), K.dyadic(gen, (2, 2, 3, 16)).to(dtype)
        bad, zero, ninf = a.clone(), a.clone(), a.clone()
        bad[0, 1, 1, 3], zero[0, 1, 1, 3], ninf[0, 1, 1, 3] = NAN, 0.0, -INF             # position 3 of window (0, 0)
        run = lambda t, g, pool: ops.relu_pool_bwd(t.cuda(), g.cuda(), pool=pool)          # noqa: E731
        assert same_bits(run(bad, d, False), run(zero, d, False)), name(dtype)
        assert same_bits(run(bad, dp, True), run(ninf, dp, True)), name(dtype)
        first = a.clone()
        first[1, 2, 4, 5] = NAN                                                           # position 0 of window (1, 2)
        dz = run(first, dp, True)
        assert not bool(dz[1, 2:4, 4:6, 5].any()) and not bool(torch.isnan(dz).any())


def test_pinned_window_codes_skip_a_nan(ops):
    """mla_conv3x3_train_codes (conv.hip code_of): strict > in scan order, so a NaN pre-activation is never chosen unless it is the
    window's first, and a window whose running maximum is NaN gets code 4 (ReLU off). Layer 6, bf16, a NaN input pixel."""
    case = K.conv_case(6, "grid")
    n, cout = K.SMALL_N, case["w"].shape[0]
    x, w, b, _, _ = N.conv_inject(case, "a", n)
    _, pre = N.conv_reference(x, w, b, True)
    codes, _ = ops.conv3x3_train_codes(x.to(BF16).cuda(), ops.repack_conv_weight(w.cuda(), BF16), b.cuda(), cout)
    assert bool(torch.isnan(pre).any()) and torch.equal(codes.cpu(), emulate_codes(pre))


def test_pinned_rn_backward_masks(ops):
    """rn_maxpool_bwd: a NaN that is not a window's first tap is never its arg-max -- the bits of the run with -inf in its place.
    rn_bn_bwd: a NaN in the kept ReLU output masks the gradient like a 0 -- the bits of the run with 0 in its place."""
    RN = importlib.import_module(PKG + ".resnet")
    x, dy, _, _ = RK.pool_case(7, 5, 8)
    bad, ninf = x.clone(), x.clone()
    bad[0, 2, 2, 1], ninf[0, 2, 2, 1] = NAN, -INF                    # (2, 2) lies in window (1, 1) only, as its centre tap
    assert same_bits(ops.rn_maxpool_bwd(bad.cuda(), dy.cuda()), ops.rn_maxpool_bwd(ninf.cuda(), dy.cuda()))
    xb, dyb, y, mean, var, gamma = RK.bn_bwd_inputs(33, 64, F32, "relu", 5, "cpu")
    bn = RN.BatchNorm2d(64).cuda()
    bn.weight.data.copy_(gamma)
    ybad, yzero = y.clone(), y.clone()
    at = (y > 0).nonzero()[7]
    ybad[at[0], at[1]], yzero[at[0], at[1]] = NAN, 0.0
    outs = [ops.rn_bn_bwd(xb.cuda(), dyb.cuda(), mean.cuda(), var.cuda(), bn, y=t.cuda())[0] for t in (ybad, yzero)]
    assert same_bits(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


def test_pinned_head_bn_backward_mask(ops, W):
    """mla_bn_bwd_* with act = 1 (mla_head.hip grad_through_act): a NaN in the kept forward output passes no gradient -- the bits
    of the run with 0 in its place."""
    mode, period, rows, cols = 0, 10, 70, 600
    x, dy, gamma, beta, keep, drop_scale = TK._bn_inputs(W, 431, rows, cols, period, 1)
    ref = TK.bn_reference(x, dy, gamma, beta, mode, period, 1, keep, drop_scale)
    y = ref["y"].float()
    at = (y > 0).nonzero()[11]
    ybad, yzero = y.clone(), y.clone()
    ybad[at[0], at[1]], yzero[at[0], at[1]] = NAN, 0.0
    outs = []
    for t in (ybad, yzero):
        dg, db = torch.empty(period, device="cuda"), torch.empty(period, device="cuda")
        dx = ops.bn_backward(x.cuda(), dy.cuda(), t.cuda(), 1, drop_scale, mode, period, ref["mean"].cuda(), ref["var"].cuda(), gamma.cuda(),
                             ops._local(), dg, db)
        outs.append((dx, dg, db))
    assert all(same_bits(a, b) and bool(torch.isfinite(a).all()) for a, b in zip(*outs))
