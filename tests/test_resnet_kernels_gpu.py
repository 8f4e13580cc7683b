"""GPU tests of the ResNet-50 trunk kernels (csrc/resnet.hip, csrc/resnet_bwd.hip, csrc/rn_core.h), ONE ops.rn_* CALL AT A TIME
against float64 torch computed from the same stored operands (for bf16: from the bf16-rounded values). The whole-trunk tests
reach these kernels with square, even-sided, post-ReLU activations under "max error over max value"; here every index
computation sees H != W, odd sizes and negative data, and every branch named in the sources is entered on its own: tiles with a
tail, the narrow and the wide column tile, the tap-less parity classes of a 1x1/2 data gradient, a split of the weight gradient
that holds one pixel, more than one BatchNorm row slice and the clamp of the slice count, the second trip of the grid-stride
loops behind grid_for(), several stem rows per block.

Two kinds of checks:
  exact    operands on a dyadic grid (multiples of 2^-3 in [-1, 1], all exact in bf16). Products are multiples of 2^-6; as long as
           sum|terms| / 2^-6 < 2^24 for an output, every partial sum in ANY order (MFMA, split-K, LDS trees) is representable in
           f32, so the kernel must equal float64 bit for bit -- and its round-to-nearest-even for bf16 outputs. Each such test
           asserts that arithmetic from its own reference before it compares with torch.equal. Max pooling and its routing
           involve no arithmetic at all.
  derived  per output element, from the float64 reference: (number of f32 roundings P, counted in the docstring) * 2^-24 *
           sum|terms|, plus rows * 2^-53 * sum|terms| where a double-precision sum feeds the result, plus half a bf16 ulp for
           bf16 outputs. No bound here is measured.

Every cap and tile constant is READ FROM THE SOURCES (grid_for's blocks x threads, kMaxSlices, the rows per slice, kTileM, the
divisor of stem_rows_per_block, the elements per LDS row), so the sizes follow the code; if a definition is rewritten, the
regular expression fails instead of leaving a branch untested. References of the cases above 16 M elements are computed with
torch float64 on the GPU, everything else on the CPU.
"""

import functools
import importlib
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import resnet50_restated as R
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                 # unit roundoff of float32
D = 2.0 ** -53                 # unit roundoff of float64
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]


def _source(name):
    with open(os.path.join(ROOT, PKG, "csrc", name)) as f:
        return f.read()


def _one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, "%s is not in the form this test reads" % what
    return found[0]


def _constants():
    core, fwd, bwd, mma = (_source(n) for n in ("rn_core.h", "resnet.hip", "resnet_bwd.hip", "mma_core.h"))
    blocks = int(_one(r"inline unsigned grid_for\(int64_t work, int64_t cap = (\d+)\) \{\s*const int64_t g = \(work \+ 255\) / 256;",
                      core, "grid_for()"))
    calls = [c for c in re.findall(r"grid_for\(([^()]*)\)", fwd + bwd)]
    assert len(calls) >= 9 and not any("," in c for c in calls), "a grid_for() call passes a cap of its own"
    slices = int(_one(r"constexpr int kMaxSlices = (\d+);", core, "kMaxSlices"))
    add, per = _one(r"const int64_t p = \(rows \+ (\d+)\) / (\d+);", core, "bn_slices()")
    assert int(add) == int(per) - 1
    tile_m = int(_one(r"constexpr int kTileM = (\d+),", core, "kTileM"))
    sadd, sdiv = _one(r"int64_t stem_rows_per_block\(int64_t rows\) \{ return \(rows \+ (\d+)\) / (\d+); \}", bwd, "stem_rows_per_block()")
    assert int(sadd) == int(sdiv) - 1
    stem_out = int(_one(r"kStemOut = (\d+),", core, "kStemOut"))
    epr = {BF16: int(_one(r"struct Elem<bf16_t> \{ static constexpr int kPerChunk = \d+, kPerRow = (\d+); \};", mma, "Elem<bf16_t>")),
           F32: int(_one(r"struct Elem<float> \{ static constexpr int kPerChunk = \d+, kPerRow = (\d+); \};", mma, "Elem<float>"))}
    return blocks * 256, slices, int(per), tile_m, int(sdiv), stem_out, epr


# threads of the largest grid (16384 x 256), kMaxSlices (512), rows per slice (2048), kTileM (128), the 1024 of
# stem_rows_per_block, kStemOut (112), elements per 128-byte LDS row (64 bf16 / 32 f32) -- as the sources stand
GRID_CAP, MAX_SLICES, SLICE_ROWS, TILE_M, STEM_BLOCKS, STEM_OUT, EPR = _constants()


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def RN():
    return importlib.import_module(PKG + ".resnet")


def name(dtype):
    return "f32" if dtype == F32 else "bf16"


def dyadic(gen, shape, bits=3, device="cpu"):
    """f32 multiples of 2^-bits in [-1, 1]: exact in bf16 for bits <= 7."""
    return torch.randint(-(1 << bits), (1 << bits) + 1, shape, generator=gen, dtype=torch.int32, device=device).float() / float(1 << bits)


def pow2_scale(gen, n, device="cpu"):
    return torch.tensor([-1.0, 0.5, 1.0, 2.0], device=device)[torch.randint(0, 4, (n,), generator=gen, device=device)]


def cast(ref64, dtype):
    """float64 -> f32 -> dtype: the value an exact f32 accumulator stores (round-to-nearest-even for bf16)."""
    return ref64.float().to(dtype)


def nchw(t):
    return t.double().permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def within(got, ref, bound, what):
    """Per-element derived bound (evaluated where the result lives); prints the worst ratio error / bound before asserting."""
    got = got.double()
    ref, bound = ref.double().to(got.device), bound.double().to(got.device)
    err = (got - ref).abs()
    assert bool(torch.isfinite(got).all()), what
    ratio = float((err / (bound + 1e-300)).max())
    print("%s: worst |error| / bound = %.3g" % (what, ratio))
    assert ratio <= 1.0, (what, ratio)


def half_ulp_bf16(ref, b32):
    """Half a bf16 ulp of any value within b32 of ref is at most 2^-9 of its binade's upper end: <= 2^-8 (|ref| + b32)."""
    return 2.0 ** -8 * (ref.abs() + b32)


# ------------------------------------------------------------------------ 1. conv forward / dgrad / wgrad: exact ----

CONV_SHAPES = [  # ks, stride, cin, cout, n, H, W -- all non-square
    (3, 1, 64, 64, 2, 5, 9),        # M = 90: less than one tile
    (1, 1, 64, 64, 3, 9, 7),        # M = 189: a full tile plus a tail
    (3, 2, 64, 128, 3, 10, 6),      # wide forward; the data gradient's parity classes hold 45 pixels
    (1, 2, 128, 64, 2, 6, 10),      # 1x1/2: three parity classes of the data gradient have no tap
    (3, 1, 192, 192, 1, 7, 5),      # three narrow column blocks forward and in the data gradient; K = 1728
    (3, 2, 192, 128, 2, 4, 8),      # narrow data gradient (Cin = 64 * 3) next to a wide forward (Cout = 128)
    (3, 1, 512, 512, 1, 4, 3),      # K = 4608 with 12 pixels: the weight gradient has one partly filled k-block, S = 1
]
assert 2 * 5 * 9 < TILE_M < 3 * 9 * 7 < 2 * TILE_M and 3 * 5 * 3 < TILE_M and 12 < min(EPR.values())


def out_hw(ks, stride, H, Wd):
    pad = ks // 2
    return (H + 2 * pad - ks) // stride + 1, (Wd + 2 * pad - ks) // stride + 1


@functools.lru_cache(maxsize=None)
def conv_case(shape):
    """Operands (f32 holders of dyadic values: the same numbers serve f32 and bf16) and the float64 references of one shape."""
    ks, stride, cin, cout, n, H, Wd = shape
    gen = torch.Generator().manual_seed(sum(p * v for p, v in zip((7919, 131, 3, 5, 17, 19, 23), shape)))
    Ho, Wo = out_hw(ks, stride, H, Wd)
    pad = ks // 2
    c = dict(x=dyadic(gen, (n, H, Wd, cin)), w=dyadic(gen, (cout, cin, ks, ks)), dy=dyadic(gen, (n, Ho, Wo, cout)),
             res_y=dyadic(gen, (n, Ho, Wo, cout)), res_x=dyadic(gen, (n, H, Wd, cin)), scale=pow2_scale(gen, cout),
             shift=dyadic(gen, (cout,)), Ho=Ho, Wo=Wo)
    x, w, dy = nchw(c["x"]), c["w"].double(), nchw(c["dy"])
    conv = lambda a, b: nhwc(F.conv2d(a, b, stride=stride, padding=pad))                                  # noqa: E731
    dgrad = lambda a, b: nhwc(conv2d_input((n, cin, H, Wd), b, a, stride=stride, padding=pad))            # noqa: E731
    wgrad = lambda a, b: conv2d_weight(a, tuple(w.shape), b, stride=stride, padding=pad)                  # noqa: E731
    c.update(y=conv(x, w), y_abs=conv(x.abs(), w.abs()), dx=dgrad(dy, w), dx_abs=dgrad(dy.abs(), w.abs()),
             dw=wgrad(x, dy), dw_abs=wgrad(x.abs(), dy.abs()))
    return c


def assert_exact_arithmetic(abs_sum, extra=0.0, unit=2.0 ** -6):
    """sum|terms| (+ what the epilogue adds) in units of the finest grid is below 2^24: every partial sum is an f32 value."""
    assert (float(abs_sum.max()) + extra) / unit < 2 ** 24, float(abs_sum.max())


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=str)
def test_conv_forward_is_exact(ops, dtype, shape):
    """rn_conv raw, with scale / shift + ReLU, with scale / shift + residual + ReLU. K <= 4608 terms of |product| <= 1 in units of
    2^-6: at most 294 912 < 2^24 (asserted from the reference). Epilogue: scale in {-1, 1/2, 1, 2} moves the grid to 2^-7 at most
    and doubles the magnitude, shift and residual are multiples of 2^-3 in [-1, 1]: (2 sum|terms| + 2) / 2^-7 < 2^24, so v * sc + sh
    is exact as two operations and as one fma. bf16 outputs are the round-to-nearest-even of that exact value."""
    ks, stride = shape[0], shape[1]
    c = conv_case(shape)
    assert_exact_arithmetic(c["y_abs"])
    assert_exact_arithmetic(2 * c["y_abs"], extra=2.0, unit=2.0 ** -7)
    x, wp = c["x"].to(dtype).cuda(), ops.rn_repack(c["w"].cuda(), dtype)
    sc, sh, res = c["scale"].cuda(), c["shift"].cuda(), c["res_y"].to(dtype).cuda()
    affine = c["y"] * c["scale"].double() + c["shift"].double()
    assert torch.equal(ops.rn_conv(x, wp, stride).cpu(), cast(c["y"], dtype)), "raw"
    assert torch.equal(ops.rn_conv(x, wp, stride, scale=sc, shift=sh, relu=True).cpu(), cast(affine.clamp_min(0), dtype)), "scale/shift + ReLU"
    got = ops.rn_conv(x, wp, stride, scale=sc, shift=sh, residual=res, relu=True)
    assert torch.equal(got.cpu(), cast((affine + c["res_y"].double()).clamp_min(0), dtype)), "residual + ReLU"


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=str)
def test_conv_dgrad_is_exact(ops, dtype, shape):
    """rn_repack_dgrad + rn_conv_dgrad, without and with the residual-path gradient. At most ks^2 Cout <= 4608 terms per element
    (a stride-2 parity class gathers a subset of the taps), + 1 for the residual, in units of 2^-6. A 1x1/2 conv reaches only the
    even positions: the other three parity classes must be the residual alone, or zero without one."""
    ks, stride, cin, cout, n, H, Wd = shape
    c = conv_case(shape)
    assert_exact_arithmetic(c["dx_abs"], extra=1.0)
    wd = ops.rn_repack_dgrad(c["w"].cuda(), dtype)
    dy, res = c["dy"].to(dtype).cuda(), c["res_x"].to(dtype).cuda()
    dx = ops.rn_conv_dgrad(dy, wd, stride, (H, Wd)).cpu()
    dxr = ops.rn_conv_dgrad(dy, wd, stride, (H, Wd), residual=res).cpu()
    assert torch.equal(dx, cast(c["dx"], dtype)), "dgrad"
    assert torch.equal(dxr, cast(c["dx"] + c["res_x"].double(), dtype)), "dgrad + residual"
    if ks == 1 and stride == 2:
        odd = torch.ones(H, Wd, dtype=torch.bool)
        odd[::2, ::2] = False
        assert not bool(dx[:, odd].any()) and torch.equal(dxr[:, odd], c["res_x"].to(dtype)[:, odd])


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=str)
def test_conv_wgrad_is_exact(ops, dtype, shape):
    """rn_conv_wgrad: n Ho Wo <= 189 terms per weight in units of 2^-6; the split partials and their sum in split order are
    exact too. dw is f32 for both dtypes."""
    ks, stride, cin, cout = shape[:4]
    c = conv_case(shape)
    assert_exact_arithmetic(c["dw_abs"])
    dw = torch.full((cout, cin, ks, ks), 9.0, device="cuda")
    ops.rn_conv_wgrad(c["x"].to(dtype).cuda(), c["dy"].to(dtype).cuda(), stride, dw)
    assert torch.equal(dw.cpu(), c["dw"].float())


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_conv_wgrad_last_split_of_one_pixel(ops, dtype):
    """3x3, 64 -> 64 on 5 x 7 x 11 = 385 pixels = 6 * 64 + 1 = 12 * 32 + 1: the plan the library reports (S splits, read from the
    workspace size) gives every split one k-block of EPR pixels, and the last split ONE pixel -- asserted from S, not assumed.
    385 terms per weight in units of 2^-6: exact."""
    shape = (3, 1, 64, 64, 5, 7, 11)
    ks, stride, cin, cout, n, H, Wd = shape
    c = conv_case(shape)
    assert_exact_arithmetic(c["dw_abs"])
    P = n * c["Ho"] * c["Wo"]
    S = int(ops._lib.lib().mla_rn_conv_wgrad_workspace_floats(n, c["Ho"], c["Wo"], cin, cout, ks, ops.DT[dtype])) // (cout * cin * ks * ks)
    kblocks = -(-P // EPR[dtype])
    kb_per = -(-kblocks // S)
    assert S > 1 and P - (S - 1) * kb_per * EPR[dtype] == 1, (S, kb_per, P)
    dw = torch.full((cout, cin, ks, ks), 9.0, device="cuda")
    ops.rn_conv_wgrad(c["x"].to(dtype).cuda(), c["dy"].to(dtype).cuda(), stride, dw)
    assert torch.equal(dw.cpu(), c["dw"].float())


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("cout,cin,ks", [(128, 64, 1), (64, 192, 3), (40, 24, 3)])
def test_repacks_are_the_permutations_of_their_header_comments(ops, dtype, cout, cin, ks):
    """rn_repack: out[o][ky][kx][i] = w[o][i][ky][kx]; rn_repack_dgrad: out[i][t][o] = w[o][i][k k - 1 - t] (taps flipped). Pure
    permutations of N(0, 1) weights: f32 bit for bit, bf16 the round-to-nearest-even of each value."""
    w = torch.randn(cout, cin, ks, ks, generator=torch.Generator().manual_seed(cout + cin + ks))
    assert torch.equal(ops.rn_repack(w.cuda(), dtype).cpu(), w.permute(0, 2, 3, 1).contiguous().to(dtype))
    assert torch.equal(ops.rn_repack_dgrad(w.cuda(), dtype).cpu(), w.flip(2, 3).permute(1, 2, 3, 0).contiguous().to(dtype))


# ------------------------------------------------------------------------------- 2. BatchNorm2d statistics ----

CONST_CH, CONST_VALUE = 5, 1.375            # exact in bf16


def bn_holder(RN, C, seed, device="cuda"):
    """A BatchNorm2d with gamma of both signs, running buffers away from (0, 1) and a batch counter that is not 0."""
    gen = torch.Generator().manual_seed(seed)
    bn = RN.BatchNorm2d(C)
    bn.weight.data.copy_((torch.rand(C, generator=gen) + 0.5) * torch.where(torch.arange(C) % 5 == 3, -1.0, 1.0))
    bn.bias.data.copy_(torch.randn(C, generator=gen) * 0.2)
    bn.running_mean.copy_(torch.randn(C, generator=gen))
    bn.running_var.copy_(torch.rand(C, generator=gen) + 0.5)
    bn.num_batches_tracked.fill_(7)
    return bn.to(device)


def stats_input(rows, C, dtype, seed, device):
    """mean 3 (c mod 7 - 3), std in [0.05, 2] by channel (a channel mix-up is visible), one constant channel."""
    gen = torch.Generator(device=device).manual_seed(seed)
    ch = torch.arange(C, device=device)
    mean, std = 3.0 * (ch % 7 - 3).float(), 0.05 + 1.95 * ((ch * 37) % 64).float() / 63.0
    x = torch.randn(rows, C, generator=gen, device=device) * std + mean
    x[:, CONST_CH] = CONST_VALUE
    return x.to(dtype)


def stats_reference(x64, bn, eps, mom):
    """float64 statistics of x64 (rows, C) and the per-element bounds.

    The kernels sum x and x^2 in double and evaluate in double: mean = s / n, var = s2 / n - mean^2, scale = gamma / sqrt(var + eps),
    shift = beta - mean scale, running = (1 - m) running + m {mean, unbiased var}; each OUTPUT is one f32 rounding of its double
    expression: 2^-24 |value| (shift: 2^-24 (|beta| + |mean scale|), the rounding of a difference that may cancel). What the double
    arithmetic itself contributes: a sum of n terms in any order is within n 2^-53 sum|terms|, so e = rows 2^-53 gives
    d_mean = e sqrt(mean^2 + var) (mean|x| <= sqrt(mean x^2)) and the one-pass variance's cancellation term d_var = e (mean^2 + var);
    scale inherits |scale| d_var / (2 (var + eps)), shift d_mean |scale| + |mean| d_scale, the running buffers m d_mean and
    m n / (n - 1) d_var."""
    rows = x64.shape[0]
    gamma, beta = bn.weight.detach().double().to(x64.device), bn.bias.detach().double().to(x64.device)
    rm, rv = bn.running_mean.double().to(x64.device), bn.running_var.double().to(x64.device)
    mean = x64.mean(dim=0)
    var = ((x64 - mean) ** 2).mean(dim=0)                     # rows = 1: exactly 0 (torch.var refuses one row)
    unb = rows / (rows - 1.0) if rows > 1 else 1.0            # ... and the unbiased factor is skipped
    scale = gamma / torch.sqrt(var + eps)
    ref = dict(mean=mean, var=var, scale=scale, shift=beta - mean * scale, running_mean=(1 - mom) * rm + mom * mean,
               running_var=(1 - mom) * rv + mom * var * unb)
    e, e2 = rows * D, mean ** 2 + var
    d_mean, d_var = e * torch.sqrt(e2), e * e2
    d_scale = scale.abs() * d_var / (2 * (var + eps))
    bound = dict(mean=U * mean.abs() + d_mean, var=U * var + d_var, scale=U * scale.abs() + d_scale,
                 shift=U * (beta.abs() + (mean * scale).abs()) + d_mean * scale.abs() + mean.abs() * d_scale,
                 running_mean=U * ref["running_mean"].abs() + mom * d_mean, running_var=U * ref["running_var"].abs() + mom * unb * d_var)
    return ref, bound


BIG_STATS_ROWS = MAX_SLICES * SLICE_ROWS + SLICE_ROWS + 5          # the slice count clamps; every block walks > 64 rows per lane
STATS_CASES = [(d, r, c) for r, c in [(1, 64), (31, 192), (SLICE_ROWS + 33, 64), (98, 2048)] for d in DTYPES] + [(F32, BIG_STATS_ROWS, 64)]


@pytest.mark.parametrize("dtype,rows,C", STATS_CASES, ids=lambda v: name(v) if isinstance(v, torch.dtype) else str(v))
def test_bn_stats_match_float64_and_both_stages_give_the_same_bits(ops, RN, dtype, rows, C):
    """rn_bn_stats, and mla_rn_bn_sums -> mla_rn_bn_finish through rn_bn_stats_sync on a one-rank group. 1 row (var 0, no unbiased
    factor), 31 rows (fewer than the 32 row lanes), two ragged slices, the smallest real layer shape (98 x 2048), and rows beyond
    kMaxSlices slices (f32 only: 269 MB). Bounds: stats_reference. The constant channel must come out with var exactly 0 and
    scale = gamma / sqrt(eps): n v / n and n v^2 / n - v^2 are exact in double for a short dyadic v. running=False leaves the
    three buffers untouched bit for bit and changes no output bit."""
    from test_resnet_dp_finetune_gpu import OneRank
    big = rows * C > 16 << 20
    x = stats_input(rows, C, dtype, 40 + rows % 1000 + C, "cuda" if big else "cpu")
    bn, idle, staged = (bn_holder(RN, C, 50 + C) for _ in range(3))
    eps, mom = float(torch.tensor(bn.eps, dtype=F32)), float(torch.tensor(bn.momentum, dtype=F32))      # the floats the C ABI receives
    ref, bound = stats_reference(x.double(), bn, eps, mom)
    before = {k: v.clone() for k, v in bn.state_dict().items()}
    xd = x.cuda()
    scale, shift, mean, var = ops.rn_bn_stats(xd, bn, running=True, want_stats=True)
    got = dict(mean=mean, var=var, scale=scale, shift=shift, running_mean=bn.running_mean, running_var=bn.running_var)
    for k in ("mean", "var", "scale", "shift", "running_mean", "running_var"):
        within(got[k], ref[k], bound[k], "rn_bn_stats %d x %d %s %s" % (rows, C, name(dtype), k))
    assert int(bn.num_batches_tracked) == 8
    assert float(var[CONST_CH]) == 0.0 and float(mean[CONST_CH]) == CONST_VALUE
    assert float(scale[CONST_CH]) == float((bn.weight.detach()[CONST_CH].double() / torch.sqrt(torch.tensor(eps, dtype=torch.float64))).float())
    if rows == 1:
        assert not bool(var.any()) and torch.equal(mean.cpu(), x[0].float())
        assert torch.equal(bn.running_var.cpu(), ((1 - mom) * before["running_var"].double().cpu()).float())
    # running=False
    out = ops.rn_bn_stats(xd, idle, running=False, want_stats=True)
    assert all(torch.equal(a, b) for a, b in zip(out, (scale, shift, mean, var)))
    assert all(torch.equal(v, before[k]) for k, v in idle.state_dict().items()), "running=False touched a buffer"
    # both stages on one rank
    rank = OneRank()
    out = ops.rn_bn_stats_sync(xd, staged, rank, running=True, want_stats=True)
    assert [t[0] for t in rank.tags] == ["syncbn_rn"]
    assert all(torch.equal(a, b) for a, b in zip(out, (scale, shift, mean, var)))
    assert all(torch.equal(v, bn.state_dict()[k]) for k, v in staged.state_dict().items())


# ----------------------------------------------------------------------------------- 3. rn_bn_eval_coeffs ----

@pytest.mark.parametrize("C", [64, 1000])
def test_bn_eval_coeffs_match_float64(ops, RN, C):
    """scale = gamma / sqrtf(rv + eps), shift = beta - rm scale in f32 (C = 1000: a partial last block of 256; running_var = 0
    included). Roundings of scale: the sum (1, halved by the square root), sqrtf (1), the division (1): 2.5, bound 3 * 2^-24 |scale|.
    shift, as two operations or one fma: |rm| times scale's error, the product (1) and the difference (1):
    2^-24 (3 |rm scale| + |rm scale| + |beta| + |rm scale|)."""
    bn = bn_holder(RN, C, 60 + C)
    bn.running_var[::9] = 0.0
    eps = float(torch.tensor(bn.eps, dtype=F32))
    gamma, beta, rm, rv = (t.detach().double().cpu() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    ref_scale = gamma / torch.sqrt(rv + eps)
    ref_shift = beta - rm * ref_scale
    scale, shift = ops.rn_bn_eval_coeffs(bn)
    prod = (rm * ref_scale).abs()
    within(scale, ref_scale, 3 * U * ref_scale.abs(), "rn_bn_eval_coeffs %d scale" % C)
    within(shift, ref_shift, U * (5 * prod + beta.abs()), "rn_bn_eval_coeffs %d shift" % C)


# ------------------------------------------------------------------------------------ 4. rn_bn_apply: exact ----

def apply_reference(x, scale, shift, res, relu):
    v = x.double() * scale.double() + shift.double()
    if res is not None:
        v = v + res.double()
    return v.clamp_min(0) if relu else v


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("rows,C", [(7, 8), (33, 192), (5, 2048)])
def test_bn_apply_is_exact(ops, dtype, rows, C):
    """y = x scale + shift [+ residual] [ReLU] on dyadic operands: x, shift, residual multiples of 2^-3 in [-1, 1], scale in
    {-1, 1/2, 1, 2} -> every intermediate is a multiple of 2^-4 below 4: exact in f32 (as two operations or one fma) and in bf16
    (6 significant bits). C = 8 is the minimum (one 16-byte chunk per row); odd row counts. out=None works in place and must give
    the out-of-place bits."""
    gen = torch.Generator().manual_seed(70 + C)
    x, res = dyadic(gen, (rows, C)).to(dtype), dyadic(gen, (rows, C)).to(dtype)
    scale, shift = pow2_scale(gen, C), dyadic(gen, (C,))
    xd, rd, sc, sh = x.cuda(), res.cuda(), scale.cuda(), shift.cuda()
    for residual, relu in ((None, False), (None, True), (rd, True)):
        ref = apply_reference(x, scale, shift, None if residual is None else res, relu)
        out = torch.full_like(xd, 9.0)
        assert ops.rn_bn_apply(xd, sc, sh, residual=residual, relu=relu, out=out) is out
        assert torch.equal(out.cpu(), cast(ref, dtype)), (residual is not None, relu)
        assert torch.equal(xd.cpu(), x), "the out-of-place call wrote its input"
        inplace = xd.clone()
        assert ops.rn_bn_apply(inplace, sc, sh, residual=residual, relu=relu) is inplace
        assert torch.equal(inplace, out), "in place"


def test_bn_apply_beyond_the_grid_cap(ops):
    """bf16, C = 64: the smallest row count whose 8-element chunks outnumber grid_for's 16384 x 256 threads (rows C / 8 = cap + 8;
    cap + 3 chunks is no whole number of 64-channel rows), so the grid-stride loop takes a second trip. 67 MB per tensor; residual
    + ReLU; the reference is the same float64 expression, evaluated on the GPU."""
    C = 64
    rows = GRID_CAP * 8 // C + 1
    assert rows * C // 8 > GRID_CAP
    gen = torch.Generator(device="cuda").manual_seed(75)
    x, res = dyadic(gen, (rows, C), device="cuda").to(BF16), dyadic(gen, (rows, C), device="cuda").to(BF16)
    scale, shift = pow2_scale(gen, C, "cuda"), dyadic(gen, (C,), device="cuda")
    out = ops.rn_bn_apply(x, scale, shift, residual=res, relu=True, out=torch.full_like(x, 9.0))
    assert torch.equal(out, cast(apply_reference(x, scale, shift, res, True), BF16))


# ----------------------------------------------------------------------- 5. rn_maxpool / rn_maxpool_bwd: exact ----

POOL_CASES = [(1, 1, 8), (1, 1, 64), (2, 3, 8), (2, 3, 64), (7, 5, 8), (7, 5, 64), (9, 112, 8), (9, 112, 64), (112, 112, 64)]


@functools.lru_cache(maxsize=None)
def pool_case(H, Wd, C):
    """All-negative quarters in [-8, -1/4] (exact in bf16; padding, were it 0, would win every border window), 3 % of the elements
    -inf, ties everywhere (32 values over 9 taps), and in image 1 a 4 x 4 corner (or the whole image) of one value: all four
    windows of pixel (1, 1) tie over all their taps. Returns x, integer dy and the float64 forward / backward of torch."""
    n = 2
    gen = torch.Generator().manual_seed(80 + H * 3 + Wd * 5 + C)
    x = -torch.randint(1, 33, (n, H, Wd, C), generator=gen).float() / 4
    x[torch.rand(n, H, Wd, C, generator=gen) < 0.03] = float("-inf")
    x[1, :4, :4] = -2.0
    Ho, Wo = (H - 1) // 2 + 1, (Wd - 1) // 2 + 1
    dy = torch.randint(-8, 9, (n, Ho, Wo, C), generator=gen).float()
    xr = nchw(x).requires_grad_(True)
    y = F.max_pool2d(xr, 3, 2, 1)
    y.backward(nchw(dy))
    assert float(y.detach().max()) < 0                                   # a padding value of 0 was never chosen
    return x, dy, nhwc(y.detach()), nhwc(xr.grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("H,Wd,C", POOL_CASES)
def test_maxpool_equals_torch_on_negative_data(ops, dtype, H, Wd, C):
    """MaxPool2d(3, 2, 1) on odd, non-square images of negative values with -inf among them: equal to F.max_pool2d."""
    x, _, y, _ = pool_case(H, Wd, C)
    got = ops.rn_maxpool(x.to(dtype).cuda())
    assert torch.equal(got.cpu().double(), y)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("H,Wd,C", POOL_CASES)
def test_maxpool_bwd_routes_like_float64_autograd(ops, dtype, H, Wd, C):
    """Integer dy in [-8, 8]: an input pixel collects at most 4 windows, every sum is exact in bf16. Ties go to the first maximum
    in torch's scan order; where every window of a pixel ties (image 1's corner), pixel (1, 1) takes window (1, 1) alone."""
    x, dy, _, dx = pool_case(H, Wd, C)
    if H >= 4 and Wd >= 4:
        assert torch.equal(dx[1, 1, 1], dy[1, 1, 1].double()) and torch.equal(dx[1, 0, 0], dy[1, 0, 0].double())
    got = ops.rn_maxpool_bwd(x.to(dtype).cuda(), dy.to(dtype).cuda())
    assert torch.equal(got.cpu().double(), dx)


def _big_pool_input(n, H, Wd, C, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return (-torch.randint(1, 33, (n, H, Wd, C), generator=gen, device="cuda").float() / 4).to(BF16)


def test_maxpool_beyond_the_grid_cap(ops):
    """bf16 (5, 3, 64) images -> (3, 2): 48 work items each, so 87 382 images outnumber the 16384 x 256 threads and the loop takes a
    second trip (168 MB in). The window of (1, 0) lies inside the image in y, the others cross a border. Reference: float64
    F.max_pool2d on the GPU."""
    H, Wd, C = 5, 3, 64
    n = GRID_CAP // (3 * 2 * C // 8) + 1
    assert n * 3 * 2 * C // 8 > GRID_CAP
    x = _big_pool_input(n, H, Wd, C, 85)
    ref = F.max_pool2d(x.double().permute(0, 3, 1, 2).contiguous(), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(ops.rn_maxpool(x).double(), ref)


def test_maxpool_bwd_beyond_the_grid_cap(ops):
    """bf16 (112, 112, 64): 100 352 work items per image, 42 images are the fewest beyond 16384 x 256 threads. Reference: float64
    autograd of F.max_pool2d on the GPU (integer dy: exact in any order)."""
    H = Wd = 112
    C = 64
    n = GRID_CAP // (H * Wd * C // 8) + 1
    assert n * H * Wd * C // 8 > GRID_CAP >= (n - 1) * H * Wd * C // 8
    x = _big_pool_input(n, H, Wd, C, 86)
    dy = torch.randint(-8, 9, (n, 56, 56, C), generator=torch.Generator(device="cuda").manual_seed(87), device="cuda").to(BF16)
    xr = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    F.max_pool2d(xr, 3, 2, 1).backward(dy.double().permute(0, 3, 1, 2).contiguous())
    assert torch.equal(ops.rn_maxpool_bwd(x, dy).double(), xr.grad.permute(0, 2, 3, 1))


# ------------------------------------------------------------------------- 6. rn_avgpool / rn_avgpool_bwd ----

def clear_of_bf16_ties(ref, slack):
    """True if no value within `slack` of ref rounds to another bf16 than ref does: then ANY f32 result within the f32 rule has
    the reference's bf16 rounding."""
    r = ref.double()
    ulp = 2.0 ** (torch.floor(torch.log2(r.abs().clamp_min(1e-30))) - 7)
    to_tie = ulp / 2 - (r - r.float().to(BF16).double()).abs()
    return bool(((to_tie > slack) | (r == 0)).all())


def check_mean(got, total64, hw, dtype, what):
    """total / hw from an exact total: bit-equal where hw is a power of two; otherwise one f32 division, 2^-24 |value| (f32
    results), and for bf16 results the round-to-nearest-even of it (asserted to be insensitive to that one rounding)."""
    ref = total64 / hw
    if hw & (hw - 1) == 0:
        assert torch.equal(got, cast(ref, dtype).to(got.device)), what
    elif dtype == F32:
        within(got, ref, U * ref.abs(), what)
    else:
        assert clear_of_bf16_ties(ref, U * ref.abs())
        assert torch.equal(got, cast(ref, dtype).to(got.device)), what


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("side,C", [(1, 100), (2, 100), (7, 100), (1, 2048), (2, 2048), (7, 2048)])
def test_avgpool_matches_float64(ops, dtype, side, C):
    """AdaptiveAvgPool2d(1) -> f32 (n, C), hw = 1, 4, 49; C = 100 is no multiple of 8. Inputs are multiples of 2^-3 in [-1, 1]: at
    most 49 * 8 units, the pixel-order sum is exact; then one division (exact for a power of two)."""
    n = 3
    x = dyadic(torch.Generator().manual_seed(90 + side + C), (n, side, side, C)).to(dtype)
    got = ops.rn_avgpool(x.cuda())
    assert got.dtype == F32
    check_mean(got.cpu(), x.double().sum(dim=(1, 2)), side * side, F32, "rn_avgpool hw %d C %d %s" % (side * side, C, name(dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_avgpool_beyond_the_grid_cap(ops, dtype):
    """hw = 4, C = 2048: n C > 16384 x 256 needs 2049 images (16.8 M elements); a power-of-two hw, so bit-equal."""
    C = 2048
    n = GRID_CAP // C + 1
    x = dyadic(torch.Generator(device="cuda").manual_seed(95), (n, 2, 2, C), device="cuda").to(dtype)
    check_mean(ops.rn_avgpool(x), x.double().sum(dim=(1, 2)), 4, F32, "rn_avgpool beyond the cap")


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("side,C", [(1, 8), (7, 8), (1, 2048), (7, 2048)])
def test_avgpool_bwd_matches_float64(ops, dtype, side, C):
    """dx (n, hw, C) = d (n, C) / hw broadcast over the pixels, d multiples of 2^-3: exact for hw = 1, one f32 division for hw = 49
    (2^-24 |value|); bf16 is the round-to-nearest-even of that."""
    n = 3
    d = dyadic(torch.Generator().manual_seed(96 + side + C), (n, C))
    got = ops.rn_avgpool_bwd(d.cuda(), (n, side, side, C), dtype)
    assert got.dtype == dtype
    total = d.double().reshape(n, 1, 1, C).expand(n, side, side, C)
    check_mean(got.cpu(), total, side * side, dtype, "rn_avgpool_bwd hw %d C %d %s" % (side * side, C, name(dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_avgpool_bwd_beyond_the_grid_cap(ops, dtype):
    """hw = 49, C = 2048: 12 544 chunks per image, 335 images are the fewest beyond 16384 x 256 threads (33.6 M elements)."""
    C, side = 2048, 7
    n = GRID_CAP // (side * side * C // 8) + 1
    assert n * side * side * C // 8 > GRID_CAP
    d = dyadic(torch.Generator(device="cuda").manual_seed(97), (n, C), device="cuda")
    got = ops.rn_avgpool_bwd(d, (n, side, side, C), dtype)
    check_mean(got, d.double().reshape(n, 1, 1, C).expand(n, side, side, C), side * side, dtype, "rn_avgpool_bwd beyond the cap")


# ------------------------------------------------------ 7. BatchNorm2d backward beyond one slice; stem gradient ----

def bn_bwd_reference(x, dy, y, mean, var, gamma, eps):
    """float64 closed form of the train-mode BatchNorm2d backward from the stored operands (x, dy, the kept ReLU output y or None,
    the statistics as handed to the kernel), on the operands' device:
      g = dy [y > 0], xhat = (x - mean) inv, inv = 1 / sqrt(var + eps), dx = gamma inv (g - mean(g) - xhat mean(g xhat)),
      dgamma = sum g xhat, dbeta = sum g, dres = g.
    Rounding count of the kernels (u = 2^-24; the sums run in double, each within rows 2^-53 sum|terms|):
      inv    = f32(1 / sqrt(double)): 1
      xhat   = (x - mean) * inv: 1 + 1 + inv's 1 = 3, each at most u (|x| + |mean|) inv = u span [the difference may cancel]
      g      exact (a select)
      dbeta  = f32(sum g): 1 -> (u + rows 2^-53) sum|g|
      dgamma = f32(sum g xhat): 3 + 1 = 4 -> (4 u + rows 2^-53) sum |g| span
      dx     = c2 (g - c0 - xhat c1) with c0 = f32(mean g) (1), c1 = f32(mean g xhat) (4), c2 = gamma * inv (2): the worst term
               xhat c1 carries 3 + 4 + 1 (product) = 8, then two differences (2) and c2 with the last product (3): 13 to first
               order, P = 14. With A = mean|g|, B = mean |g| span every term is below T = |gamma| inv (|g| + A + span B).
      bf16 outputs add half a bf16 ulp (half_ulp_bf16)."""
    rows = x.shape[0]
    x64, d64 = x.double(), dy.double()
    g = d64 if y is None else torch.where(y.double() > 0, d64, torch.zeros_like(d64))
    mean, var, gamma = mean.double(), var.double(), gamma.double()
    inv = 1.0 / torch.sqrt(var + eps)
    xh = (x64 - mean) * inv
    ref = dict(dx=gamma * inv * (g - g.mean(dim=0) - xh * (g * xh).mean(dim=0)), dgamma=(g * xh).sum(dim=0), dbeta=g.sum(dim=0), dres=g)
    span, ga = (x64.abs() + mean.abs()) * inv, g.abs()
    A, B = ga.mean(dim=0), (ga * span).mean(dim=0)
    bound = dict(dx=14 * U * gamma.abs() * inv * (ga + A + span * B), dbeta=(U + rows * D) * A * rows, dgamma=(4 * U + rows * D) * B * rows)
    if x.dtype == BF16:
        bound["dx"] = bound["dx"] + half_ulp_bf16(ref["dx"], bound["dx"])
    return ref, bound


def bn_bwd_inputs(rows, C, dtype, mode, seed, device):
    """x with per-channel mean and spread, its float64 batch statistics rounded to f32 (what the forward hands on), dy ~ N(0, 1),
    gamma of both signs, and the forward output y = [relu](xhat gamma + beta [+ residual]) rounded to the dtype."""
    gen = torch.Generator(device=device).manual_seed(seed)
    ch = torch.arange(C, device=device)
    x = (torch.randn(rows, C, generator=gen, device=device) * (0.5 + (ch % 5).float() * 0.4) + (ch % 7 - 3).float()).to(dtype)
    dy = torch.randn(rows, C, generator=gen, device=device).to(dtype)
    gamma = (torch.rand(C, generator=gen, device=device) + 0.5) * torch.where(ch % 5 == 3, -1.0, 1.0)
    beta = torch.randn(C, generator=gen, device=device) * 0.2
    x64 = x.double()
    mean = x64.mean(dim=0)
    var = ((x64 - mean) ** 2).mean(dim=0)
    y = None
    if mode != "plain":
        v = (x64 - mean) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double()
        if mode == "relu_residual":
            v = v + torch.randn(rows, C, generator=gen, device=device).to(dtype).double()
        y = v.clamp_min(0).float().to(dtype)
    return x, dy, y, mean.float(), var.float(), gamma


def run_bn_bwd(ops, RN, x, dy, y, mean, var, gamma, mode, what):
    C = x.shape[1]
    bn = RN.BatchNorm2d(C).cuda()
    bn.weight.data.copy_(gamma)
    eps = float(torch.tensor(bn.eps, dtype=F32))
    ref, bound = bn_bwd_reference(x, dy, y, mean, var, gamma, eps)
    dgamma, dbeta = torch.full((C,), 9.0, device="cuda"), torch.full((C,), 9.0, device="cuda")
    dx, dres = ops.rn_bn_bwd(x.cuda(), dy.cuda(), mean.cuda(), var.cuda(), bn, y=None if y is None else y.cuda(),
                             want_dres=mode == "relu_residual", dgamma=dgamma, dbeta=dbeta)
    within(dx, ref["dx"], bound["dx"], what + " dx")
    within(dgamma, ref["dgamma"], bound["dgamma"], what + " dgamma")
    within(dbeta, ref["dbeta"], bound["dbeta"], what + " dbeta")
    if mode == "relu_residual":
        assert torch.equal(dres.cpu(), cast(ref["dres"], x.dtype).cpu()), what + " dres"
    else:
        assert dres is None
    return ref


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("mode", ["plain", "relu", "relu_residual"])
@pytest.mark.parametrize("rows,C", [(SLICE_ROWS + 33, 64), (3136, 192)])
def test_bn_bwd_beyond_one_slice_matches_float64(ops, RN, dtype, mode, rows, C):
    """rn_bn_bwd with P = 2 row slices (ragged: 2048 + 33 rows; 3136 = 56 x 56 rows of layer1 at 3 column groups): the slice order
    of bn_sum_slices at kernel level. Bounds: bn_bwd_reference. The closed form is first checked against float64 autograd of
    F.batch_norm on the batch's own float64 statistics."""
    assert -(-rows // SLICE_ROWS) == 2
    x, dy, y, mean, var, gamma = bn_bwd_inputs(rows, C, dtype, mode, 100 + rows + len(mode), "cpu")
    ref = run_bn_bwd(ops, RN, x, dy, y, mean, var, gamma, mode, "rn_bn_bwd %d x %d %s %s" % (rows, C, mode, name(dtype)))
    # the closed form IS the gradient: autograd through the batch statistics, float64 throughout
    xr, gr = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    out = F.batch_norm(xr, None, None, gr, torch.zeros(C, dtype=torch.float64), training=True, eps=1e-5)
    out.backward(ref["dres"])
    m64 = x.double().mean(dim=0)
    exact, _ = bn_bwd_reference(x, dy, y, m64, ((x.double() - m64) ** 2).mean(dim=0), gamma, 1e-5)
    assert float((exact["dx"] - xr.grad).abs().max()) < 1e-11 and float((exact["dgamma"] - gr.grad).abs().max()) < 1e-9


def test_bn_bwd_beyond_the_grid_cap(ops, RN):
    """bf16, C = 64, ReLU + residual: rows C / 8 chunks just beyond grid_for's 16384 x 256 threads, so rn_bn_bwd_apply_kernel takes
    a second trip (and the sums run over 257 slices). 67 MB per tensor; the reference is the closed form in float64 on the GPU."""
    C = 64
    rows = GRID_CAP * 8 // C + 1
    assert rows * C // 8 > GRID_CAP and 2 < -(-rows // SLICE_ROWS) < MAX_SLICES
    x, dy, y, mean, var, gamma = bn_bwd_inputs(rows, C, BF16, "relu_residual", 110, "cuda")
    run_bn_bwd(ops, RN, x, dy, y, mean, var, gamma, "relu_residual", "rn_bn_bwd beyond the cap")


@functools.lru_cache(maxsize=None)
def stem_case(conf, n):
    """Planes in [0, 1), dy ~ N(0, 1) rounded to bf16 (one reference serves both dtypes), float64 conv2d_weight of the normalised
    input (tests/resnet50_restated.py)."""
    gen = torch.Generator().manual_seed(120 + n)
    planes = torch.rand(n, 224, 224, generator=gen)
    dy = torch.randn(n, STEM_OUT, STEM_OUT, 64, generator=gen).to(BF16)
    xn = R.normalize_input(planes.double().reshape(n, 1, 1, 224, 224), conf)
    return planes, dy, conv2d_weight(xn, (64, 3, 7, 7), nchw(dy), stride=2, padding=3)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("conf", ["repeat", "single"])
@pytest.mark.parametrize("n", [10, 19])
def test_stem_wgrad_with_several_rows_per_block(ops, dtype, conf, n):
    """rn_stem_wgrad at 10 and 19 images: 1120 and 2128 output rows, so stem_rows_per_block is 2 and 3; 112 rows per image are no
    multiple of 3, so blocks cross image boundaries, and 2128 = 709 * 3 + 1 leaves the last block a single row. The bound is the
    one-row-per-block test's (tests/test_resnet_finetune_gpu.py): max error over max value 1e-4 (f32) / 1e-2 (bf16)."""
    rows = n * STEM_OUT
    rpb = -(-rows // STEM_BLOCKS)
    assert rpb == {10: 2, 19: 3}[n] and (STEM_OUT % rpb != 0 or n == 10) and (n == 10 or rows % rpb == 1)
    planes, dy, ref = stem_case(conf, n)
    dw = torch.full((64, 3, 7, 7), 9.0, device="cuda")
    ops.rn_stem_wgrad(planes.cuda(), conf == "single", dy.to(dtype).cuda(), dw)
    e = float((dw.double().cpu() - ref).abs().max() / ref.abs().max())
    print("rn_stem_wgrad %s n %d %s: max error over max value %.3g" % (conf, n, name(dtype), e))
    assert e <= (1e-4 if dtype == F32 else 1e-2)
