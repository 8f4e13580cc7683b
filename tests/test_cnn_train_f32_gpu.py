"""GPU tests of the f32 VGGish backward kernels (csrc/cnn_train.hip with the rules it shares with the bf16 form in
csrc/cnn_train_core.h, the f32 dgrad instantiations of csrc/conv.hip), one kernel at a time against float64 torch autograd on the CPU.

Most tests here need NO tolerance: operands are drawn from a coarse dyadic grid (multiples of 2^-4 in [-1, 1] unless a test says
otherwise). A product of two grid values is a multiple of 2^-8, and as long as the sum of the absolute values of all terms of one
output, divided by that unit, stays below 2^24, every partial sum in ANY order (MFMA, fma chains, shuffle trees, split
reductions) is exactly representable in float32 -- the kernel must then equal the float64 reference bit for bit. Each docstring
states that arithmetic. Exact ties are frequent on such data, which is the point for the pooling kernels: they must follow torch's
first-maximum-in-scan-order rule and relu'(0) = 0.
"""

import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PKG

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(64, 128, 48, 32), (128, 256, 24, 16), (256, 256, 24, 16), (256, 512, 12, 8), (512, 512, 12, 8)]   # conv2..conv6: cin, cout, H, W


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


def grid(W, seed, stream, shape, bits=4, lo=-1.0, hi=1.0):
    """Uniform values rounded to multiples of 2^-bits (float32, exact)."""
    v = W.uniform(seed, stream, int(np.prod(shape)), lo=lo, hi=hi, dtype=np.float64)
    return torch.from_numpy(np.round(v * 2.0 ** bits) / 2.0 ** bits).float().reshape(shape)


def big_grid(gen, shape, bits=4):
    """The same kind of values for the large cases (torch's generator: tens of millions of elements in a fraction of a second)."""
    return torch.randint(-(1 << bits), (1 << bits) + 1, shape, generator=gen, dtype=torch.int32).float() / float(1 << bits)


def nchw(t):
    return t.double().permute(0, 3, 1, 2)


def pool_reference(a, d, pool):
    """float64 autograd of max_pool2d(relu(a), 2) (or relu(a)) at NHWC a: (forward output, dA), both NHWC."""
    x = nchw(a).clone().requires_grad_(True)
    y = F.max_pool2d(F.relu(x), 2) if pool else F.relu(x)
    y.backward(nchw(d))
    return y.detach().permute(0, 2, 3, 1), x.grad.permute(0, 2, 3, 1)


def plant(a):
    """One window of four equal positive values (the first position must win) and one all-zero window (nothing may flow)."""
    a[0, :2, :2, :] = 0.5
    a[1, 2:4, 2:4, :] = 0.0
    return a


@pytest.mark.parametrize("n,H,Wd,C", [(3, 12, 8, 512), (3, 48, 32, 128)])
def test_maxpool_and_relu_pool_bwd_f32_equal_torch(ops, W, n, H, Wd, C):
    """mla_maxpool2x2, mla_relu_pool_bwd and mla_relu_pool_bwd_bias in f32, pooled and un-pooled. No arithmetic but the bias
    gradient's column sum: at most n H W = 4608 terms of |value| <= 1 in units of 2^-4 -> |sum| / unit <= 73 728 < 2^24, exact
    (the kernel sums in double anyway). Everything else is selection: equality with torch, ties and zeros included."""
    a = plant(grid(W, 801, C, (n, H, Wd, C)).clamp_min(0))              # post-ReLU: about half zeros, 17 distinct values
    pooled_ref, _ = pool_reference(a, torch.zeros(n, H // 2, Wd // 2, C), True)
    assert torch.equal(ops.maxpool2x2(a.cuda()).cpu().double(), pooled_ref)
    for pool in (True, False):
        d = grid(W, 802 + pool, C, (n, H // 2, Wd // 2, C) if pool else (n, H, Wd, C))
        _, dz_ref = pool_reference(a, d, pool)
        if pool:
            # torch's rule on the planted windows: the first of four equal values takes everything, zeros take nothing
            assert torch.equal(dz_ref[0, 0, 0], d[0, 0, 0].double()) and not bool(dz_ref[0, 0, 1].any() or dz_ref[0, 1, :2].any())
            assert not bool(dz_ref[1, 2:4, 2:4].any())
        dz = ops.relu_pool_bwd(a.cuda(), d.cuda(), pool=pool)
        assert torch.equal(dz.cpu().double(), dz_ref), "relu_pool_bwd pool=%s" % pool
        db = torch.full((C,), 9.0, device="cuda")
        dz = ops.relu_pool_bwd(a.cuda(), d.cuda(), pool=pool, db=db)
        assert torch.equal(dz.cpu().double(), dz_ref), "relu_pool_bwd_bias pool=%s" % pool
        assert torch.equal(db.cpu().double(), dz_ref.sum(dim=(0, 1, 2))), "bias gradient pool=%s" % pool


def test_relu_bwd_f32_of_the_last_linear_layer(ops, W):
    """The Linear form: a (40, 128) activation, un-pooled, with and without the bias gradient (40 terms per column: exact)."""
    h, g = grid(W, 805, 1, (40, 128)).clamp_min(0), grid(W, 806, 1, (40, 128))
    ref = torch.where(h > 0, g, torch.zeros_like(g))
    assert torch.equal(ops.relu_pool_bwd(h.cuda(), g.cuda(), pool=False).cpu(), ref)
    db = torch.full((128,), 9.0, device="cuda")
    assert torch.equal(ops.relu_pool_bwd(h.cuda(), g.cuda(), pool=False, db=db).cpu(), ref)
    assert torch.equal(db.cpu().double(), ref.double().sum(dim=0))


def test_relu_pool_bwd_bias_f32_grid_stride_loop(ops):
    """relu_pool_bwd_kernel<true> (the form with bias slots) always runs 4096 x 256 threads: pooled (48, 24, 16, 256) has 1 179 648 work items, so 131 072 threads
    take a second trip and their slots hold two elements. db: 48 * 12 * 8 = 4608 terms per channel, exact as above."""
    gen = torch.Generator().manual_seed(811)
    n, H, Wd, C = 48, 24, 16, 256
    assert n * (H // 2) * (Wd // 2) * C > 4096 * 256
    a, d = plant(big_grid(gen, (n, H, Wd, C)).clamp_min(0)), big_grid(gen, (n, H // 2, Wd // 2, C))
    _, dz_ref = pool_reference(a, d, True)
    db = torch.full((C,), 9.0, device="cuda")
    dz = ops.relu_pool_bwd(a.cuda(), d.cuda(), pool=True, db=db)
    assert torch.equal(dz.cpu().double(), dz_ref) and torch.equal(db.cpu().double(), dz_ref.sum(dim=(0, 1, 2)))


def test_relu_pool_bwd_f32_beyond_the_grid_cap(ops):
    """mla_relu_pool_bwd caps its grid at 16384 blocks of 256: 342 images of (12, 8, 512) are 4 202 496 pooled work items
    (un-pooled: 16.8 M), so the grid-stride loop runs in both forms."""
    gen = torch.Generator().manual_seed(812)
    n, H, Wd, C = 342, 12, 8, 512
    assert n * (H // 2) * (Wd // 2) * C > 16384 * 256
    a = plant(big_grid(gen, (n, H, Wd, C)).clamp_min(0))
    for pool in (True, False):
        d = big_grid(gen, (n, H // 2, Wd // 2, C) if pool else (n, H, Wd, C))
        _, dz_ref = pool_reference(a, d, pool)
        assert torch.equal(ops.relu_pool_bwd(a.cuda(), d.cuda(), pool=pool).cpu().double(), dz_ref), pool


def test_maxpool_f32_beyond_the_grid_cap(ops):
    """maxpool_kernel<float> works on four channels per thread, so its 16384 x 256 cap is passed only above 4 194 304 output QUADS: 1366
    images of (12, 8, 512). No shape passes that cap with less than 4 x 4 194 304 x 4 input values (268 MB of f32): the channel
    count cancels. The float64 reference is taken in slices of 128 images, so the host holds 50 MB of it at a time."""
    gen = torch.Generator().manual_seed(813)
    n, H, Wd, C = 1366, 12, 8, 512
    assert n * (H // 2) * (Wd // 2) * (C // 4) > 16384 * 256
    a = big_grid(gen, (n, H, Wd, C))
    got = ops.maxpool2x2(a.cuda()).cpu()
    for i in range(0, n, 128):
        ref = F.max_pool2d(a[i:i + 128].double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        assert torch.equal(got[i:i + 128].double(), ref), i


def _wgrad_reference(a, dz):
    x64 = nchw(a).contiguous()
    w64 = torch.zeros((dz.shape[3], a.shape[3], 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, w64, padding=1).backward(nchw(dz).contiguous())
    return w64.grad


WGRAD_CASES = [(s, 3) for s in SHAPES] + [((256, 512, 12, 8), 25), ((512, 512, 12, 8), 13)]


@pytest.mark.parametrize("shape,n", WGRAD_CASES)
def test_wgrad_f32_equals_float64_on_grid_values(ops, W, shape, n):
    """mla_conv_wgrad on v_mfma_f32_16x16x4_f32, all five compiled shapes at 3 images (3 splits), and splits + 1 images for the two
    12 x 8 layers (splits = ceil(768 / tiles) = 24 and 12: the per-split image loop then runs unevenly, split 0 takes two images).
    dW = sum over n H W pixels of dZ * A: at most 3 * 48 * 32 = 4608 (or 25 * 96 = 2400) products of |value| <= 1 in units of
    2^-8 -> |sum| / unit <= 1.2e6 < 2^24: every partial sum is exact, the result equals float64 autograd of F.conv2d."""
    cin, cout, H, Wd = shape
    a, dz = grid(W, 821, cin + n, (n, H, Wd, cin)), grid(W, 822, cout + n, (n, H, Wd, cout))
    dw = torch.full((cout, cin, 3, 3), 9.0, device="cuda")
    ops.conv_wgrad(dz.cuda(), a.cuda(), dw)
    assert torch.equal(dw.cpu().double(), _wgrad_reference(a, dz))


@pytest.mark.parametrize("shape", SHAPES)
def test_wgrad_f32_on_uniform_values_within_the_derived_bound(ops, W, shape):
    """The same kernel on uniform random values: P = n H W products plus the split reduction, so every dW element is within
    (n H W + splits) * 2^-24 * sum|dZ A| of float64 (sum of absolute terms from the same autograd on absolute values). The
    launcher takes splits = min(ceil(768 / tiles), n) with at most 64 tiles, so 3 images are 3 splits at every shape. The bound is
    loose (a worst case over 2300 to 4600 roundings); the grid-value cases above are the sharp ones."""
    cin, cout, H, Wd = shape
    n = splits = 3
    a = torch.from_numpy(W.uniform(823, cin, n * H * Wd * cin, lo=-0.5, hi=1.5)).reshape(n, H, Wd, cin)
    dz = torch.from_numpy(W.uniform(824, cout, n * H * Wd * cout)).reshape(n, H, Wd, cout)
    dw = torch.empty((cout, cin, 3, 3), device="cuda")
    ops.conv_wgrad(dz.cuda(), a.cuda(), dw)
    ref, terms = _wgrad_reference(a, dz), _wgrad_reference(a.abs(), dz.abs())
    ratio = float(((dw.cpu().double() - ref).abs() / ((n * H * Wd + splits) * U * terms)).max())
    print("wgrad %s uniform: worst |error| / bound = %.3g" % (shape, ratio))
    assert ratio <= 1.0, ratio


def test_wgrad_refuses_a_shape_that_is_not_compiled(ops):
    a, dz = torch.zeros((1, 24, 16, 64), device="cuda"), torch.zeros((1, 24, 16, 128), device="cuda")
    dw = torch.full((128, 64, 3, 3), 9.0, device="cuda")
    with pytest.raises(ops._lib.MlaError) as e:
        ops.conv_wgrad(dz, a, dw)
    assert e.value.code == -2 and "not compiled" in str(e.value)
    assert bool((dw == 9.0).all())


DGRAD_SHAPES = [(512, 512, 12, 8), (512, 256, 12, 8), (256, 256, 24, 16), (256, 128, 24, 16), (128, 64, 48, 32)]


@pytest.mark.parametrize("cin,cout,H,Wd", DGRAD_SHAPES)
def test_dgrad_f32_equals_float64_conv_transpose(ops, W, cin, cout, H, Wd):
    """repack_dgrad(f32) + conv3x3(act=False): the five transposed convolutions of the backward pass, dA[ci] = sum over 9 taps and
    cout_fwd channels of dZ * W flipped. At most 9 * 512 = 4608 products in units of 2^-8, |sum| / unit <= 1.2e6 < 2^24: exact,
    equal to F.conv_transpose2d in float64. Here `cin` is the forward layer's Cout (the channels of dZ)."""
    n = 3
    dz = grid(W, 831, cin, (n, H, Wd, cin))
    wf = grid(W, 832, cout, (cin, cout, 3, 3))                          # forward weight (Cout_fwd = cin, Cin_fwd = cout)
    got = ops.conv3x3(dz.cuda(), ops.repack_dgrad(wf.cuda(), torch.float32), None, cout, pool=False, act=False)
    ref = F.conv_transpose2d(nchw(dz), wf.double(), padding=1).permute(0, 2, 3, 1)
    assert torch.equal(got.cpu().double(), ref)


@pytest.mark.parametrize("cin,cout,H,Wd", DGRAD_SHAPES)
def test_dgrad_f32_on_uniform_values_within_the_derived_bound(ops, W, cin, cout, H, Wd):
    """The same path on uniform random values, where the low mantissa bits of every product count: dA[ci] is a sum of 9 * cin
    products (`cin` = channels of dZ), so it is within 9 cin * 2^-24 * sum|dZ W| of float64 (the sum of absolute terms is the same
    transposed convolution of the absolute values)."""
    n = 3
    dz = torch.from_numpy(W.uniform(833, cin, n * H * Wd * cin)).reshape(n, H, Wd, cin)
    wf = torch.from_numpy(W.uniform(834, cout, cin * cout * 9, lo=-0.5, hi=1.5)).reshape(cin, cout, 3, 3)
    got = ops.conv3x3(dz.cuda(), ops.repack_dgrad(wf.cuda(), torch.float32), None, cout, pool=False, act=False)
    ref = F.conv_transpose2d(nchw(dz), wf.double(), padding=1).permute(0, 2, 3, 1)
    terms = F.conv_transpose2d(nchw(dz.abs()), wf.double().abs(), padding=1).permute(0, 2, 3, 1)
    ratio = float(((got.cpu().double() - ref).abs() / (9 * cin * U * terms)).max())
    print("dgrad %s uniform: worst |error| / bound = %.3g" % ((cin, cout, H, Wd), ratio))
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("n", [3, 172])
def test_conv1_bwd_f32_equals_autograd_on_grid_values(ops, W, n):
    """mla_conv1_bwd recomputes conv1 + ReLU + max-pool per pooled pixel and reduces dW (64 x 9) and db (64) in f32 registers,
    wave shuffles and per-block partials. 172 clips are 1032 blocks of 256 pooled pixels > the 1024-block cap: the grid-stride loop
    runs. Grid: x multiples of 1/4 in [-2, 2], w and bias multiples of 1/8 in [-1, 1] / [-0.5, 0.5], d_pooled multiples of 1/4 in [-1, 1].
      forward: 9 products in units of 2^-5, |sum + bias| <= 18.5 -> exact in any order (fma chain here, conv2d there); the
               arg-max over the window and the `best + bias > 0` threshold see the same numbers as torch, ties included
      dW:      n * 1536 = 264 192 terms |g x| <= 2 in units of 2^-4 -> |sum| / unit <= 8.5e6 < 2^24
      db:      264 192 terms |g| <= 1 in units of 2^-2 -> 1.1e6 < 2^24
    so dW and db equal float64 autograd of max_pool2d(relu(conv2d)) exactly, and two calls give the same bits."""
    x = grid(W, 841, n, (n, 96, 64), bits=2, lo=-2.0, hi=2.0)
    w, b = grid(W, 842, 1, (64, 1, 3, 3), bits=3), grid(W, 843, 1, (64,), bits=3, lo=-0.5, hi=0.5)
    d = grid(W, 844, n, (n, 48, 32, 64), bits=2)
    outs = []
    for _ in range(2):
        dw, db = torch.full((64, 1, 3, 3), 9.0, device="cuda"), torch.full((64,), 9.0, device="cuda")
        ops.conv1_bwd(x.cuda(), w.cuda(), b.cuda(), d.cuda(), dw, db)
        outs.append((dw.cpu(), db.cpu()))
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    for i in range(0, n, 43):                                            # the reference in chunks of 43 clips (memory)
        y = F.max_pool2d(F.relu(F.conv2d(x[i:i + 43].double()[:, None], w64, b64, padding=1)), 2)
        y.backward(nchw(d[i:i + 43]))
    assert torch.equal(outs[0][0].double(), w64.grad) and torch.equal(outs[0][1].double(), b64.grad)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
