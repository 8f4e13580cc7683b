"""GPU tests of the inference conv and GEMM kernels (csrc/conv.hip, csrc/gemm.hip), ONE KERNEL CALL AT A TIME -- through ops, or
through _lib where a pitch or a guard region is needed -- against float64 torch computed from the same stored operands (for bf16:
from the bf16-rounded values). The whole-model tests reach these kernels under "max error over max value" and with batches in
which no persistent workgroup takes a second tile; here every output element is compared, the conv batches are large enough
that a workgroup re-uses both of its LDS patch buffers, and every tile form of dispatch<> is entered on its own, named by its id.

Two kinds of checks:
  exact    operands (and biases) on a dyadic grid: multiples of 2^-3 in [-1, 1], all exact in bf16. Products are multiples of 2^-6;
           as long as sum|terms| / 2^-6 < 2^24 for an output, every partial sum in ANY order (MFMA, K ranges, ring stages) is
           representable in f32, so f32 outputs must equal float64 bit for bit and bf16 outputs its round-to-nearest-even. Every
           such test asserts that arithmetic from its own reference. The bf16x3 mode needs a non-zero lo plane: its operands are
           sparse multiples of 2^-9 (hi = bf16(x) and lo = x - hi both exact), the unit is 2^-18, and the reference is the
           three-product sum a_hi w_hi + a_hi w_lo + a_lo w_hi of the stored planes (the kernel drops a_lo w_lo by design). Split
           outputs are compared plane by plane: hi = bf16(v), lo = bf16(v - hi).
  derived  uniform random inputs. Per output element: (number of f32 roundings P, counted in the docstring) * 2^-24 * sum|terms|,
           plus half a bf16 ulp for bf16 outputs. No bound here is measured.

Shapes, operand builders, references and the constants READ FROM THE SOURCES live in tests/infer_kernel_cases.py (they evaluate
without a device: tests/test_infer_kernel_cases_cpu.py). References above a few million elements are computed with torch float64
on the GPU, the 13-image conv references wherever a device is available.

Status: written and collected without a GPU; not yet run on the MI355X (DESIGN.md section 4 says the same).
"""

import ctypes
import importlib
import os

import pytest
import torch

import infer_kernel_cases as K
from conftest import PKG
from infer_kernel_cases import BF16, F32, U, cast, name, split_out, within

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
SENTINEL = -7.0                          # exact in bf16; no ReLU output, and no padding value, equals it


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def code(L, dtype):
    return L.F32 if dtype == F32 else L.BF16


def ptr(t):
    return vp(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------------------ 1. conv2..conv6: exact, all images ----

def run_conv(ops, layer, mode, n):
    """One ops.conv call on n images (the 13 distinct ones repeated cyclically) against the reference of the 13."""
    c = K.conv_case(layer, "sparse9" if mode == "bf16x3" else "grid")
    x13, wp, y13 = K.conv_operands(c, mode)
    idx = torch.arange(n, device="cuda") % K.P_IMAGES
    x = x13.cuda()[idx].contiguous()
    got = ops.conv(layer, x, wp.cuda(), c["b"].cuda(), split=mode == "bf16x3")
    want = y13.cuda()[idx]
    if not torch.equal(got, want):
        bad = (got != want).flatten(1).any(dim=1).nonzero().flatten()
        raise AssertionError("conv%d %s, %d images: %d images differ, the first at index %d (image %d of the cycle)"
                             % (layer, mode, n, bad.numel(), int(bad[0]), int(bad[0]) % K.P_IMAGES))


@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16x3"])
@pytest.mark.parametrize("layer", K.LAYERS)
def test_conv_small_batch_is_exact(ops, layer, mode):
    """n = 5: a tail in the 4-image W = 8 tiles and in the image pairs of the 2 x 4-wave W = 8 tiles. At most 9 * 512 = 4608 terms of
    |product| <= 1 plus the bias, in units of 2^-6 (grid) or 2^-18 (sparse 2^-9 operands): below 2^24, asserted by conv_case()."""
    run_conv(ops, layer, mode, K.SMALL_N)


@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16x3"])
@pytest.mark.parametrize("layer", K.LAYERS)
def test_conv_persistent_batch_is_exact(ops, cus, layer, mode):
    """More than 2 * (2 cus / n_tiles_n) tiles, so some persistent workgroup takes a third tile: both LDS-DMA patch buffers are re-used
    (halo rows zeroed once), patch_rsrc is rebuilt per tile, and the batch ends inside a tile (imgs_here < IMGS) where tiles hold
    several images. Every image is compared; an index that is wrong by anything but a multiple of 13 images shows."""
    g = K.conv_cfg(layer, mode, "tall")
    run_conv(ops, layer, mode, K.persistent_n(g, cus))


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("layer", K.LAYERS)
def test_conv_wide_tiles_persistent_batch_is_exact(ops, cus, layer, mode):
    """The same with MLA_CONV_TILE=wide: the 192-pixel tiles of the bf16 modes get a reference of their own."""
    g = K.conv_cfg(layer, mode, "wide")
    assert "MLA_CONV_TILE" not in os.environ
    os.environ["MLA_CONV_TILE"] = "wide"
    try:
        run_conv(ops, layer, mode, K.persistent_n(g, cus))
    finally:
        os.environ.pop("MLA_CONV_TILE", None)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("layer", [3, 6])
def test_conv_writes_nothing_past_the_batch(L, layer, mode):
    """One W = 16 layer and one W = 8 layer (5 images: the last tile is partly absent): the image behind the batch keeps its sentinel
    and the last real image is exact."""
    c = K.conv_case(layer, "sparse9" if mode == "bf16x3" else "grid")
    x13, wp, y13 = K.conv_operands(c, mode)
    n = K.SMALL_N
    x, wp, b = x13[:n].contiguous().cuda(), wp.cuda(), c["b"].cuda()
    out = torch.full((n + 1,) + tuple(y13.shape[1:]), SENTINEL, dtype=BF16, device="cuda")
    L.check(L.lib().mla_vggish_conv(layer, ptr(x), ptr(wp), ptr(b), ptr(out), n, L.BF16X3 if mode == "bf16x3" else L.BF16, L.stream_ptr()))
    assert bool((out[n] == SENTINEL).all()), "wrote past the batch"
    assert torch.equal(out[n - 1].cpu(), y13[n - 1]) and torch.equal(out[:n].cpu(), y13[:n])


# ------------------------------------------------------------------------------------------------------ 3. conv1 ----

def conv1_ns(cus):
    return (3, K.conv1_persistent_n(cus))


@pytest.mark.parametrize("pair", K.CONV1_PAIRS + ["split"], ids=lambda p: p if p == "split" else "%s-%s" % (name(p[0]), name(p[1])))
def test_conv1_is_exact(ops, cus, pair):
    """mla_vggish_conv1 with grid log-mel values and a grid filter: 9 terms + bias in units of 2^-6, exact in f32 and in bf16 operands.
    3 clips, and a count beyond the persistent caps of conv1_kernel and conv1_patch_kernel with a remainder against both; every clip
    of the 13-clip cycle is compared. Split form: f32 input -> [hi(64) | lo(64)] bf16 planes of the exact value."""
    c = K.conv1_case("grid")
    y, y_abs = K.conv1_reference(c["x"], c["w"], c["b"])
    K.assert_exact_arithmetic(y_abs)
    x_dtype, out_dtype = (F32, BF16) if pair == "split" else pair
    want13 = (split_out(y) if pair == "split" else cast(y, out_dtype)).cuda()
    for n in conv1_ns(cus):
        idx = torch.arange(n, device="cuda") % K.P_IMAGES
        x = c["x"].to(x_dtype).cuda()[idx].contiguous()
        got = ops.conv1(x, c["w"].cuda(), c["b"].cuda(), out_dtype, split=pair == "split")
        assert torch.equal(got, want13[idx]), n


@pytest.mark.parametrize("pair", K.CONV1_PAIRS + ["split"], ids=lambda p: p if p == "split" else "%s-%s" % (name(p[0]), name(p[1])))
def test_conv1_within_derived_bound(ops, cus, pair):
    """Uniform data. f32 outputs (conv1_kernel, three v_mfma_f32_16x16x4_f32 per pixel, internal order unknown -- worst case): 9
    product roundings + 9 additions into the accumulator + the bias addition: P = 19. bf16 outputs (conv1_patch_kernel): the kernel
    multiplies bf16(x) by bf16(w) -- the reference is built from those rounded operands --, bf16 products are exact in f32, the
    accumulator starts at the bias and takes 9 non-zero terms: P = 9, plus half a bf16 ulp. Pooling and ReLU do not widen a bound
    (the largest bound of a window holds for its maximum). Split: P = 19 on the merged value hi + lo, plus the rounding of lo,
    |lo| <= 2^-8 |v| rounded to 2^-8 relative: 2^-16 (|ref| + bound)."""
    c = K.conv1_case("uniform")
    x_dtype, out_dtype = (F32, F32) if pair == "split" else pair
    x = c["x"].to(x_dtype)
    rounds = K.conv1_rounds_operands_to_bf16(x_dtype, out_dtype)
    y, y_abs = K.conv1_reference(x.to(BF16) if rounds else x, c["w"].to(BF16) if rounds else c["w"], c["b"])
    bound = (9 if rounds else 19) * U * y_abs
    if out_dtype == BF16:
        bound = bound + K.half_ulp_bf16(y, bound)
    if pair == "split":
        bound = bound + 2.0 ** -16 * (y.abs() + bound)
    for n in conv1_ns(cus):
        idx = torch.arange(n, device="cuda") % K.P_IMAGES
        got = ops.conv1(x.cuda()[idx].contiguous(), c["w"].cuda(), c["b"].cuda(), BF16 if pair == "split" else out_dtype, split=pair == "split")
        if pair == "split":
            got = got[..., :64].double() + got[..., 64:].double()
        within(got, y.cuda()[idx], bound.cuda()[idx], "conv1 %s, %d clips" % (pair if pair == "split" else name(x_dtype) + "->" + name(out_dtype), n))


# ---------------------------------------------------------------------------------------------------- 4. helpers ----

@pytest.mark.parametrize("dtype", [F32, BF16], ids=name)
@pytest.mark.parametrize("cout,cin", [(128, 64), (5, 3)])
def test_repack_conv_weight(ops, dtype, cout, cin):
    w = torch.randn((cout, cin, 3, 3), generator=torch.Generator().manual_seed(cout))
    assert torch.equal(ops.repack_conv_weight(w.cuda(), dtype).cpu(), K.packed_weight(w, dtype))


def test_to_bf16_and_to_f32(ops, ):
    """Against torch's own casts, bit for bit: ties to even, +-0, the largest finite values, subnormals; then beyond the 8192 x 256 grid."""
    x = torch.cat([K.special_f32(), torch.randn(K.C["helper_cap"] + 333, generator=torch.Generator().manual_seed(3))])
    got = ops.to_bf16(x.cuda())
    assert torch.equal(got.cpu().view(torch.int16), x.to(BF16).view(torch.int16))
    assert torch.equal(ops.to_f32(got).cpu().view(torch.int32), x.to(BF16).float().view(torch.int32))


SPLIT_CASES = [  # rows, cols, seg, copies, extra input pitch, extra output pitch
    (7, 192, 64, 2, 0, 0), (7, 192, 64, 3, 0, 0), (5, 96, 32, 2, 8, 24), (5, 96, 32, 3, 8, 24), (3, 40, 40, 3, 4, 0),
    (2051, 1024, 256, 2, 0, 0), (1027, 2048, 512, 3, 8, 8),
]
assert 2051 * 1024 > K.C["helper_cap"] and 1027 * 2048 > K.C["helper_cap"]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=str)
def test_split_bf16x3(L, case):
    """mla_split_bf16x3 against hi = bf16(x), lo = bf16(x - hi) as torch rounds them, [hi | lo (| hi)] per segment; padding columns of
    the input hold large values that must not be read as data, those of the output a sentinel that must survive."""
    rows, cols, seg, copies, pad_in, pad_out = case
    x = torch.randn((rows, cols), generator=torch.Generator().manual_seed(rows + cols))
    src = torch.full((rows, cols + pad_in), 1024.0)
    src[:, :cols] = x
    src, out = src.cuda(), torch.full((rows, copies * cols + pad_out), SENTINEL, dtype=BF16, device="cuda")
    L.check(L.lib().mla_split_bf16x3(ptr(src), rows, cols, cols + pad_in, ptr(out), copies * cols + pad_out, seg, copies, L.stream_ptr()))
    out = out.cpu()
    assert torch.equal(out[:, :copies * cols], K.split_reference(x, seg, copies)) and bool((out[:, copies * cols:] == SENTINEL).all())


@pytest.mark.parametrize("case", [(7, 192, 64, 0), (5, 96, 32, 24), (3, 40, 40, 8), (2051, 1024, 256, 0), (1027, 2048, 512, 8)], ids=str)
def test_merge_bf16x3(L, case):
    """mla_merge_bf16x3 = hi + lo in ONE f32 addition, per segment, from planes that are NOT a split (any two bf16 values)."""
    rows, cols, seg, pad_in = case
    p = torch.randn((rows, 2 * cols), generator=torch.Generator().manual_seed(rows)).to(BF16)
    src = torch.full((rows, 2 * cols + pad_in), 1024.0, dtype=BF16)
    src[:, :2 * cols] = p
    src, out = src.cuda(), torch.full((rows + 1, cols), SENTINEL, device="cuda")
    L.check(L.lib().mla_merge_bf16x3(ptr(src), rows, cols, 2 * cols + pad_in, seg, ptr(out), L.stream_ptr()))
    assert torch.equal(out[:rows].cpu(), K.merge_reference(p, seg)) and bool((out[rows] == SENTINEL).all())


# --------------------------------------------------------------------------------------- 5./6. GEMM forms: exact ----

def check_form(case_id, M, N, kk, dtype, cus):
    form = K.gemm_form(M, N, kk, K.KPR[dtype], cus)
    assert form == K.form_of(case_id), "on %d CUs a %d x %d x %d %s GEMM runs the %s form, not the one this case is named after" % (
        cus, M, N, kk, name(dtype), form)


@pytest.mark.parametrize("pair", K.GEMM_PAIRS, ids=lambda p: "%s-%s" % (name(p[0]), name(p[1])))
@pytest.mark.parametrize("case_id", list(K.GEMM_CASES))
def test_linear_form_is_exact(ops, cus, case_id, pair):
    """ops.linear in the tile form the id names (asserted with the device's CU count), M = tile rows * k + 5, a partly empty last
    column tile, the smallest K that keeps the form: with bias and ReLU, with bias and no ReLU, and without a bias. K <= 9 * 64 terms
    + bias in units of 2^-6, asserted from the reference."""
    dtype, out_dtype = pair
    M, N, _ = K.GEMM_CASES[case_id]
    kk = K.gemm_k(case_id, dtype)
    check_form(case_id, M, N, kk, dtype, cus)
    a, w, b = K.gemm_operands(M + N + kk, M, N, kk, device="cuda")
    y, y_abs = K.gemm_reference(a, w, b)
    K.assert_exact_arithmetic(y_abs)
    a, w = a.to(dtype), w.to(dtype)
    assert torch.equal(ops.linear(a, w, b, relu=True, out_dtype=out_dtype), cast(y.clamp_min(0), out_dtype)), "bias + ReLU"
    assert torch.equal(ops.linear(a, w, b, relu=False, out_dtype=out_dtype), cast(y, out_dtype)), "bias"
    assert torch.equal(ops.linear(a, w, None, relu=False, out_dtype=out_dtype), cast(y - b.double(), out_dtype)), "no bias"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=name)
@pytest.mark.parametrize("case_id", list(K.GEMM_DERIVED))
def test_linear_form_within_derived_bound(ops, cus, case_id, dtype):
    """Uniform operands in [-1, 1), K = 2048, f32 -> f32 and bf16 -> bf16. The matrix unit's internal order is not documented -- worst
    case: f32: one rounding per product and one per addition (K products, K additions, the bias): P = 2K + 1. bf16: products of bf16
    values are exact in f32: P = K + 1, plus half a bf16 ulp for the store. (No term passes through more than K + 1 of these
    roundings, so P u sum|terms| also covers the second-order terms of (1 + u)^depth.)"""
    M, N = K.GEMM_DERIVED[case_id]
    kk = 2048
    check_form(case_id, M, N, kk, dtype, cus)
    gen = torch.Generator(device="cuda").manual_seed(M)
    a, w = (torch.rand(s, generator=gen, device="cuda") * 2 - 1 for s in ((M, kk), (N, kk)))
    b = torch.rand((N,), generator=gen, device="cuda") - 0.5
    a, w = a.to(dtype), w.to(dtype)
    y, y_abs = K.gemm_reference(a, w, b)
    bound = ((2 * kk + 1) if dtype == F32 else (kk + 1)) * U * y_abs
    if dtype == BF16:
        bound = bound + K.half_ulp_bf16(y, bound)
    within(ops.linear(a, w, b, relu=False), y, bound, "%s %s" % (case_id, name(dtype)))


# -------------------------------------------------------------------------------------------------- 7. pitches ----

@pytest.mark.parametrize("pair", K.GEMM_PAIRS, ids=lambda p: "%s-%s" % (name(p[0]), name(p[1])))
@pytest.mark.parametrize("case_id", ["64x128/reg", "64x128/dma"])
def test_linear_with_row_pitches(L, cus, case_id, pair):
    """mla_linear with lda > K, ldw > K, ldo > N: the padding of a and w holds 1024 (one leaked value would be visible in any output), K
    ends inside a 128-byte row in the register-staged twin; the padding of out and a guard row keep their sentinel. Exact."""
    dtype, out_dtype = pair
    M, N, _ = K.GEMM_CASES[case_id]
    kk = K.gemm_k(case_id, dtype)
    check_form(case_id, M, N, kk, dtype, cus)
    lda, ldw, ldo = kk + 3 * K.PER[dtype], kk + K.PER[dtype], N + 5
    a, w, b = K.gemm_operands(11, M, N, kk, device="cuda")
    y, y_abs = K.gemm_reference(a, w, b)
    K.assert_exact_arithmetic(y_abs)
    ap, wp = torch.full((M, lda), 1024.0, dtype=dtype, device="cuda"), torch.full((N, ldw), 1024.0, dtype=dtype, device="cuda")
    ap[:, :kk], wp[:, :kk] = a.to(dtype), w.to(dtype)
    out = torch.full((M + 1, ldo), SENTINEL, dtype=out_dtype, device="cuda")
    L.check(L.lib().mla_linear(ptr(ap), lda, ptr(wp), ldw, ptr(b), ptr(out), ldo, M, N, kk, code(L, dtype), code(L, out_dtype), 0, L.stream_ptr()))
    assert torch.equal(out[:M, :N], cast(y, out_dtype)), "values"
    assert bool((out[:M, N:] == SENTINEL).all()) and bool((out[M] == SENTINEL).all()), "padding of out"


# ------------------------------------------------------------------------------------------- 8. K ranges ----

def workspace(n):
    return torch.full((n,), float("nan"), device="cuda")


@pytest.mark.parametrize("pair", K.GEMM_PAIRS, ids=lambda p: "%s-%s" % (name(p[0]), name(p[1])))
@pytest.mark.parametrize("shape", [(133, 100, 1), (133, 100, 3), (8200, 128, 1)], ids=str)
def test_linear_ksplit_is_exact(L, shape, pair):
    """mla_linear_ksplit with ops.KSPLIT (8) ranges of one and of three 128-byte rows each, M and N tails; 8200 x 128 outputs are more
    than splitk_reduce_kernel's 4096 x 256 threads: the second trip of its grid-stride loop. The workspace starts as NaN."""
    dtype, out_dtype = pair
    M, N, rows = shape
    S = K.C["ksplit"]
    kk = K.KPR[dtype] * S * rows
    assert (M * N > K.C["reduce_cap"]) == (M == 8200)
    a, w, b = K.gemm_operands(M + rows, M, N, kk, device="cuda")
    y, y_abs = K.gemm_reference(a, w, b)
    K.assert_exact_arithmetic(y_abs)
    a, w = a.to(dtype), w.to(dtype)
    for relu in (True, False):
        out, ws = torch.full((M, N), SENTINEL, dtype=out_dtype, device="cuda"), workspace(S * M * N)
        L.check(L.lib().mla_linear_ksplit(ptr(a), kk, ptr(w), kk, ptr(b), ptr(out), N, M, N, kk, code(L, dtype), code(L, out_dtype), int(relu), S,
                                          ptr(ws), ws.numel(), L.stream_ptr()))
        assert torch.equal(out, cast(y.clamp_min(0) if relu else y, out_dtype)), relu


@pytest.mark.parametrize("case", [("lib", 133, 100, 256, 2), ("lib", 133, 100, 768, 2), ("ops", 133, 100, 2048, 4), ("ops", 133, 100, 32768, 64),
                                  ("ops", 700, 300, 4096, 8)], ids=str)
def test_linear_splitk_is_exact(ops, L, case):
    """mla_linear_splitk, f32. ops.linear(split_k=True) chooses min(64, max(2, 256 // tiles), K // 512) ranges with tiles <= 64 and
    K >= 2048, i.e. 4 ... 64: both ends and one in between through ops (the count is asserted from that formula), and the library's
    own minimum of 2 ranges through _lib at K = 8 and 24 rows of 128 bytes. 32768 terms in units of 2^-6: 2 097 152 < 2^24."""
    via, M, N, kk, splits = case
    a, w, b = K.gemm_operands(kk, M, N, kk, device="cuda")
    y, y_abs = K.gemm_reference(a, w, b)
    K.assert_exact_arithmetic(y_abs)
    if via == "ops":
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        assert tiles <= 64 and kk >= 2048 and min(64, max(2, 256 // tiles), kk // 512) == splits
        assert torch.equal(ops.linear(a, w, b, relu=True, split_k=True), cast(y.clamp_min(0), F32))
        return
    out, ws = torch.full((M, N), SENTINEL, device="cuda"), workspace(splits * M * N)
    L.check(L.lib().mla_linear_splitk(ptr(a), kk, ptr(w), kk, ptr(b), ptr(out), N, M, N, kk, 0, splits, ptr(ws), ws.numel(), L.stream_ptr()))
    assert torch.equal(out, cast(y, F32))


# --------------------------------------------------------------------------------------------- 9. bf16x3 GEMM ----

@pytest.mark.parametrize("out_split", [False, True], ids=["f32", "split"])
@pytest.mark.parametrize("case_id", list(K.X3_GEMM_CASES))
def test_linear_bf16x3_is_exact(ops, cus, case_id, out_split):
    """mla_linear_bf16x3 in the 64 x 128, 128 x 128 and ring forms (3K bf16 columns reach dispatch<>), segments of 64 and of K / 2
    columns, M and N tails, against the three-product reference of the stored planes; sparse 2^-9 operands, sum|terms| / 2^-18 < 2^24
    asserted. f32 output, and split output compared plane by plane."""
    M, N, kk, seg = K.X3_GEMM_CASES[case_id]
    form = K.gemm_form(M, N, 3 * kk, K.KPR[BF16], cus)
    assert form.split("/")[0] == case_id.split("-")[0], "on %d CUs this case runs the %s form" % (cus, form)
    c = K.x3_gemm_case(M + kk + seg, M, N, kk)
    K.assert_exact_arithmetic(c["y_abs"], 2.0 ** -18)
    a2, w3, b = K.seg_planes_a(c["a"], seg).cuda(), K.seg_planes_w(c["w"], seg).cuda(), c["b"].cuda()
    for relu in (True, False):
        y = c["y"].clamp_min(0) if relu else c["y"]
        got = ops.linear_split(a2, w3, b, seg, relu=relu, out_split=out_split).cpu()
        assert torch.equal(got, split_out(y) if out_split else cast(y, F32)), relu
