"""GPU tests of the bf16 VGGish finetune kernels (csrc/cnn_train_bf16.hip with the rules of csrc/cnn_train_core.h, and the bf16 forms of
csrc/conv.hip's generic conv entry), ONE KERNEL CALL AT A TIME against float64 torch computed from the same stored operands.

No tolerance is used here. Operands lie on a dyadic grid that bf16 holds exactly; every test takes sum|terms| per output element from
its float64 reference and asserts max sum|terms| / unit < 2^24. Then every partial sum in ANY order is an f32 value -- MFMA
accumulators, per-split partials, wgrad_reduce_kernel's f32 sum over the splits, the sRed adds of conv1's backward -- and the result
must be torch.equal to the reference (bf16 outputs: to its round-to-nearest-even). That is a condition on the data, asserted from the
reference alone, not a measurement. Exact ties are frequent on such data, which is the point for the routing kernels: first maximum
in scan order, relu'(0) = 0.

Shapes, operand builders, references and the constants READ FROM THE SOURCES live in tests/cnn_train_bf16_cases.py; they evaluate
without a device (tests/test_cnn_train_bf16_cases_cpu.py, at 256 CUs). tests/test_finetune_bf16_gpu.py keeps the uniform-data and
composed checks.

Status: written and collected without a GPU, references and planted cases evaluated on the CPU; not yet run on the MI355X
(DESIGN.md section 4 says the same)."""

import ctypes
import importlib
import os

import pytest
import torch

import cnn_train_bf16_cases as T
import infer_kernel_cases as K
from conftest import PKG
from infer_kernel_cases import BF16

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ptr(t):
    return vp(t.data_ptr()) if t is not None else None


def cyclic(t13, n):
    return t13.cuda()[torch.arange(n, device="cuda") % K.P_IMAGES].contiguous()


def wide_tiles():
    """MLA_CONV_TILE=wide for the calls inside the `with` block, restored afterwards."""
    class _Wide:
        def __enter__(self):
            assert "MLA_CONV_TILE" not in os.environ
            os.environ["MLA_CONV_TILE"] = "wide"

        def __exit__(self, *exc):
            os.environ.pop("MLA_CONV_TILE", None)
    return _Wide()


class _Tall:
    def __enter__(self):
        assert "MLA_CONV_TILE" not in os.environ

    def __exit__(self, *exc):
        pass


def tiles(tile):
    return wide_tiles() if tile == "wide" else _Tall()


# ------------------------------------------------------------------------------------------- 1. conv_wgrad ----

def _wgrad_ids():
    return [cid for cid, _, _ in T.wgrad_cases(T.CUS_ASSUMED)]


@pytest.mark.parametrize("cid", _wgrad_ids())
def test_wgrad_bf16_is_exact(ops, cus, cid):
    """wgrad_bf16_kernel + wgrad_reduce_kernel. The image count of a case is worked out from the device's CU count (splits = CUs /
    tiles): n = 3 (one image per workgroup), n = splits + 1 (split 0 takes two images: the per-split image loop, uneven n_mine, and
    for BANDS > 1 the hand-over from an image's last band to the next image's band 0 in the other LDS buffer, where the y-halo
    re-zero must clear what an earlier item left), n = 2 splits + 1 for W = 8 (three items in a BANDS == 1 workgroup: both LDS
    images re-used), n = 1 (fewer images than splits). Values are multiples of 2^-2 in [-1, 1] (n <= 3: of 2^-4), products
    multiples of 2^-4 (2^-8): sum|terms| / unit <= n H W * 16 <= 257 * 1536 * 16 = 6.3e6 < 2^24 even with every |term| = 1 --
    asserted from the reference's own sum|terms|. Rows 0 and H - 1 of the input of split 0's images are 1.0. Reference: float64
    autograd of F.conv2d on the CPU up to 17 images, beyond that nine shifted float64 matmuls on the device (the CPU file proves the
    two forms equal bit for bit)."""
    shape, n = {c: (s, m) for c, s, m in T.wgrad_cases(cus)}[cid]
    cin, cout, H, Wd = shape
    big = n > 17
    a, dz, unit = T.wgrad_operands(shape, n, cus, device="cuda" if big else "cpu")
    ref = T.wgrad_matmul(a, dz) if big else T.wgrad_autograd(a, dz)
    T.assert_exact(T.wgrad_matmul(a.cuda(), dz.cuda(), absolute=True), unit)
    dw = torch.full((cout, cin, 3, 3), 9.0, device="cuda")
    ops.conv_wgrad(dz.cuda().to(BF16), a.cuda().to(BF16), dw)
    assert torch.equal(dw.double(), ref.cuda()), "%s, %d images: %d of %d elements differ" % (cid, n, int((dw.double() != ref.cuda()).sum()), dw.numel())


# ---------------------------------------------------------------------------------------------- 2. conv1_bwd ----

@pytest.mark.parametrize("n", T.CONV1_NS)
def test_conv1_bwd_bf16_is_exact(ops, n):
    """conv1_bwd_mfma_kernel + conv1_bwd_mfma_finish_kernel against float64 autograd of max_pool2d(relu(conv2d)). x multiples of 2^-2
    in [-1, 3], w of 2^-4 in [-1/2, 1/2], bias of 2^-4, d_pooled of 2^-3 in [-1, 1]: all exact in bf16, so the kernel's f2bf changes
    nothing, and the recompute (bias + 9 products in units of 2^-6, |sum| <= 14) is exact on both sides: the routing is identical
    INCLUDING ties -- the tie rule (first maximum wins), the `> 0` ReLU edge and the tap index arithmetic of the finish kernel are
    checked bit for bit. The planted cases (constant block of x, zero filter with positive / zero bias, a single-tap channel that
    puts the maximum on every position) are asserted on the reference's own routing in conv1_bwd_reference.
      n = 1: 12 workgroups;  n = 3;  n = 65: n_seg = 3120 > 4 kC1MaxWg = 3072, so 48 waves take a second row.
      dW: at most n * 1536 = 99 840 terms |g x| <= 3 in units of 2^-5 -> <= 9.6e6 < 2^24; db: |g| <= 1 in units of 2^-3 -> 8e5.
    Both asserted from the reference's sum|terms|."""
    if n == 65:
        assert n * 48 > 4 * T.C["c1_max_wg"]
    x, w, b, d = T.conv1_bwd_operands(n)
    dw_ref, db_ref, dw_abs, db_abs = T.conv1_bwd_reference(x, w, b, d)
    T.assert_exact(dw_abs, 2.0 ** -5)
    T.assert_exact(db_abs, 2.0 ** -3)
    dw, db = torch.full((64, 1, 3, 3), 9.0, device="cuda"), torch.full((64,), 9.0, device="cuda")
    ops.conv1_bwd(x.cuda(), w.cuda(), b.cuda(), d.cuda().to(BF16), dw, db)
    assert torch.equal(db.cpu().double(), db_ref), "db: channels %s differ" % (db.cpu().double() != db_ref).nonzero().flatten().tolist()
    assert torch.equal(dw.cpu().double(), dw_ref), "dW: channels %s differ" % (dw.cpu().double() != dw_ref).flatten(1).any(dim=1).nonzero().flatten().tolist()


# ------------------------------------------------------------------------------- 3. pool / ReLU backward ----

def _bias_ws(ops):
    return ops._bias_ws(True, torch.device("cuda", torch.cuda.current_device()))


@pytest.mark.parametrize("pool", [True, False], ids=["pooled", "unpooled"])
@pytest.mark.parametrize("shape", T.POOL_SHAPES, ids=str)
def test_relu_pool_bwd_bf16_is_exact(ops, L, shape, pool):
    """relu_pool_bwd_bf16_kernel<bf16, bf16> always launches kBiasGrid8 x 256 lanes of 8 channels. (2, 4, 6, 8) and (3, 2, 2, 16): C / 8
    = 1 and 2, tensors smaller than the grid. (172, 12, 8, 512): pooled 264 192 work items against 262 144 lanes, so 2048 lanes take a
    second trip and their bias slots hold two elements; un-pooled more than four trips. Selection only, plus the bias gradient: at most
    172 * 96 terms of |value| <= 1 in units of 2^-3 (summed in double): db equals the float64 column sum of the reference dZ. dZ
    equals float64 autograd (first maximum, relu'(0) = 0; planted windows asserted in pool_reference). The image behind the tensor
    and db are pre-filled with a sentinel: the image must keep it."""
    n, H, Wd, Cc = shape
    lanes = T.C["bias_grid8"] * 256
    if n > 100:
        assert (lanes < n * (H // 2) * (Wd // 2) * Cc // 8 < 2 * lanes) if pool else (n * H * Wd * Cc // 8 > 4 * lanes)
    a, d = T.pool_operands(shape, pool)
    dz_ref = T.pool_reference(a, d, pool)
    T.assert_exact(dz_ref.abs().sum(dim=(0, 1, 2)), 2.0 ** -3)
    dz = torch.full((n + 1, H, Wd, Cc), T.SENTINEL, dtype=BF16, device="cuda")
    db = torch.full((Cc,), 9.0, device="cuda")
    ag, dg = a.cuda().to(BF16), d.cuda().to(BF16)
    L.check(L.lib().mla_relu_pool_bwd_bf16(ptr(ag), L.BF16, ptr(dg), L.BF16, ptr(dz), n, H, Wd, Cc, int(pool), ptr(_bias_ws(ops)), ptr(db), L.stream_ptr()))
    assert bool((dz[n] == T.SENTINEL).all()), "wrote past the tensor"
    assert torch.equal(dz[:n].cpu().double(), dz_ref)
    assert torch.equal(db.cpu().double(), dz_ref.sum(dim=(0, 1, 2)))
    assert torch.equal(ops.relu_pool_bwd(ag, dg, pool=pool), dz[:n])                # the form without the bias slots: same dZ


@pytest.mark.parametrize("shape", T.POOL_SHAPES, ids=str)
def test_pool_bwd_codes_bf16_is_exact(ops, L, shape):
    """pool_bwd_codes_bf16_kernel against the plain rule dz[window position code] = d where code < 4, 0 elsewhere (route_by_codes),
    codes uniform in 0..4 (the entry's contract). Eight consecutive channels of one pixel hold 0, 1, 2, 3, 4, 3, 2, 1 with eight
    distinct gradients: the byte order inside the two 32-bit code words. Same shapes as above (C / 8 = 1, 2; a second trip of the
    grid-stride loop); db (code-4 elements excluded) is an exact double sum; the image behind the tensor keeps its sentinel."""
    n, H, Wd, Cc = shape
    codes, d = T.codes_operands(shape)
    dz_ref = T.route_by_codes(codes, d)
    dz = torch.full((n + 1, H, Wd, Cc), T.SENTINEL, dtype=BF16, device="cuda")
    db = torch.full((Cc,), 9.0, device="cuda")
    cg, dg = codes.cuda(), d.cuda().to(BF16)
    L.check(L.lib().mla_pool_bwd_codes_bf16(ptr(cg), ptr(dg), ptr(dz), n, H, Wd, Cc, ptr(_bias_ws(ops)), ptr(db), L.stream_ptr()))
    assert bool((dz[n] == T.SENTINEL).all()), "wrote past the tensor"
    assert torch.equal(dz[:n].cpu().double(), dz_ref)
    assert torch.equal(db.cpu().double(), dz_ref.sum(dim=(0, 1, 2)))
    assert torch.equal(ops.pool_bwd_codes(cg, dg), dz[:n])


# ------------------------------------------------------------------------- 4. the bf16 generic conv entry ----

def _packed(ops, w):
    return ops.repack_conv_weight(w.cuda(), BF16)


@pytest.mark.parametrize("layer", T.FWD_LAYERS)
def test_conv3x3_bf16_unpooled_forward_is_exact(ops, layer):
    """ops.conv3x3(pool=False, act=True) in bf16 at every VGGish shape (layers 3 and 5 are what the finetune step runs through this
    entry, 2, 4, 6 the kept-activation forms), 5 images of infer_kernel_cases.conv_case's grid operands (multiples of 2^-3, planted
    borders and corners): at most 9 * 512 products + bias in units of 2^-6, below 2^24 (asserted by conv_case). The output is the
    round-to-nearest-even of relu(exact pre-activation)."""
    c = K.conv_case(layer, "grid")
    n = K.SMALL_N
    got = ops.conv3x3(c["x"][:n].cuda().to(BF16), _packed(ops, c["w"]), c["b"].cuda(), c["w"].shape[0], pool=False, act=True)
    assert torch.equal(got.cpu(), K.cast(c["pre"][:n].clamp_min(0), BF16))


def _run_dgrad(ops, shape, n):
    c = T.dgrad_case(shape)
    wd = ops.repack_dgrad(c["wf"].cuda(), BF16)
    assert torch.equal(wd.cpu(), c["wf"].flip(2, 3).permute(1, 2, 3, 0).reshape(shape[1], 9, shape[0]).to(BF16))
    got = ops.conv3x3(cyclic(c["dz"].to(BF16), n), wd, None, shape[1], pool=False, act=False)
    want = cyclic(K.cast(c["y"], BF16), n)
    if not torch.equal(got, want):
        bad = (got != want).flatten(1).any(dim=1).nonzero().flatten()
        raise AssertionError("dgrad %s, %d images: %d images differ, the first at index %d" % (shape, n, bad.numel(), int(bad[0])))


@pytest.mark.parametrize("shape", T.DGRAD_SHAPES, ids=str)
def test_dgrad_bf16_is_exact(ops, shape):
    """repack_dgrad(bf16) + conv3x3(act=False): the five transposed convolutions of the backward pass at 5 images, the special tall
    128 -> 64 tile among them. dA = sum over 9 taps and the channels of dZ: at most 4608 products in units of 2^-6 (asserted in
    dgrad_case); bf16 output = round-to-nearest-even of F.conv_transpose2d in float64. The repacked weight is the flipped,
    transposed filter itself."""
    _run_dgrad(ops, shape, K.SMALL_N)


@pytest.mark.parametrize("shape", T.WIDE_DGRAD, ids=str)
def test_dgrad_bf16_wide_tiles_is_exact(ops, shape):
    """One W = 16 and one W = 8 dgrad shape on the 192-pixel tiles (MLA_CONV_TILE=wide)."""
    with wide_tiles():
        _run_dgrad(ops, shape, K.SMALL_N)


@pytest.mark.parametrize("shape", T.PERSISTENT_DGRAD, ids=str)
def test_dgrad_bf16_persistent_batch_is_exact(ops, cus, shape):
    """A batch in which some persistent workgroup takes a third tile (both LDS patch buffers re-used), counted as
    infer_kernel_cases.persistent_n does, for the 128 -> 64 tall tile and for one W = 8 form; every image is compared."""
    _run_dgrad(ops, shape, K.persistent_n(T.generic_cfg(*shape, "tall"), cus))


@pytest.mark.parametrize("layer", T.POOLED_LAYERS)
def test_conv3x3_train_bf16_is_exact(ops, layer):
    """mla_conv3x3_train in bf16 on the grid operands: the kept pre-pool activation is the round-to-nearest-even of relu(exact
    pre-activation), the pooled output that of the window maximum -- against the float64 reference, not against the composition of
    two other kernels."""
    c = K.conv_case(layer, "grid")
    n = K.SMALL_N
    a, p = ops.conv3x3_train(c["x"][:n].cuda().to(BF16), _packed(ops, c["w"]), c["b"].cuda(), c["w"].shape[0])
    prepool, pooled, _codes, _ties, _top = T.train_reference(c["pre"][:n])
    assert torch.equal(a.cpu(), prepool) and torch.equal(p.cpu(), pooled) and torch.equal(pooled, K.cast(c["y"][:n], BF16))


CODE_CASES = [(l, "tall") for l in T.POOLED_LAYERS] + [(l, "wide") for l in T.WIDE_LAYERS if l in T.POOLED_LAYERS]


@pytest.mark.parametrize("layer,tile", CODE_CASES)
def test_conv3x3_train_codes_equal_the_reference(ops, layer, tile):
    """mla_conv3x3_train_codes: every code is the first maximum in scan order of the four EXACT pre-activations, or 4 where that maximum
    is <= 0. Two operand sets, 5 images each. 'grid' (conv_case): long exact sums. 'narrow' (narrow_case): x multiples of 2^-1, four
    non-zero weights per output channel, |pre-activation| <= 5 in units of 2^-2 -- at least 1 % of the windows tie for the maximum
    and some maximum is exactly 0 (both asserted here and on the CPU), so `a1 > a0` against `a1 >= a0` and `> 0` against `>= 0`
    decide thousands of codes. End to end on the narrow set, where every pre-activation is a bf16 value and the stored pre-pool
    activation therefore orders a window exactly as the accumulators do: pool_bwd_codes(codes, d) equals
    relu_pool_bwd(prepool, d, pool=True) ELEMENT FOR ELEMENT, and both equal the reference routing. (On the grid set the two
    forms legitimately differ where distinct pre-activations round to one bf16 value; there the codes alone are checked.)"""
    n = K.SMALL_N
    for kind in ("grid", "narrow"):
        c = K.conv_case(layer, "grid") if kind == "grid" else T.narrow_case(layer)
        cout = c["w"].shape[0]
        prepool, pooled, codes_ref, ties, top = T.train_reference(c["pre"][:n])
        if kind == "narrow":
            assert float(ties.double().mean()) >= 0.01 and bool((top == 0).any())
        x, wp, b = c["x"][:n].cuda().to(BF16), _packed(ops, c["w"]), c["b"].cuda()
        with tiles(tile):
            codes, p = ops.conv3x3_train_codes(x, wp, b, cout)
            a, p2 = (ops.conv3x3_train(x, wp, b, cout) if kind == "narrow" else (None, p))
        differ = codes.cpu() != codes_ref
        assert not bool(differ.any()), "%s: %d codes differ, %d of them in tied windows" % (kind, int(differ.sum()), int((differ & ties).sum()))
        assert torch.equal(p.cpu(), pooled) and torch.equal(p2, p)
        if kind == "narrow":
            assert torch.equal(a.cpu(), prepool)
            d = K.dyadic(torch.Generator().manual_seed(layer), tuple(codes_ref.shape))
            dz_ref = T.route_by_codes(codes_ref, d)
            db_c, db_a = torch.full((cout,), 9.0, device="cuda"), torch.full((cout,), 9.0, device="cuda")
            dz_c = ops.pool_bwd_codes(codes, d.cuda().to(BF16), db=db_c)
            dz_a = ops.relu_pool_bwd(a, d.cuda().to(BF16), pool=True, db=db_a)
            assert torch.equal(dz_c, dz_a) and torch.equal(dz_c.cpu().double(), dz_ref)
            assert torch.equal(db_c, db_a) and torch.equal(db_c.cpu().double(), dz_ref.sum(dim=(0, 1, 2)))
