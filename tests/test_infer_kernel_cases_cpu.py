"""CPU side of tests/test_infer_kernels_gpu.py: the case table reaches every tile form of gemm.hip's dispatch<> at 256 CUs, the image
counts of the conv cases do make a persistent workgroup take a third tile, and every operand builder, float64 reference and exactness
assertion of the GPU file evaluates without a device (at the small sizes)."""

import pytest
import torch

import infer_kernel_cases as K
from infer_kernel_cases import BF16, F32

CUS = 256


def test_case_table_reaches_every_gemm_form_at_256_cus():
    forms = {"64x128", "128x128", "ring", "128x256", "256x256", "256x256+128", "320x256"}
    reached = set()
    for cid, (M, N, _rows) in K.GEMM_CASES.items():
        for dtype in (F32, BF16):
            kk = K.gemm_k(cid, dtype)
            assert kk % K.PER[dtype] == 0
            assert K.gemm_form(M, N, kk, K.KPR[dtype], CUS) == K.form_of(cid), (cid, K.name(dtype))
            reached.add(K.form_of(cid))
    # every form LDS-DMA, and register-staged where that exists: the ring and the 320 x 256 tile are LDS-DMA only
    assert reached == {f + "/dma" for f in forms} | {f + "/reg" for f in forms - {"ring", "320x256"}}
    for cid, (M, N) in K.GEMM_DERIVED.items():
        for dtype in (F32, BF16):
            want = "ring/dma" if cid == "ring/dma" else cid
            assert K.gemm_form(M, N, 2048, K.KPR[dtype], CUS) == want, cid
    assert {c.split("/")[0] for c in K.GEMM_DERIVED} == forms
    for cid, (M, N, kk, seg) in K.X3_GEMM_CASES.items():
        assert K.gemm_form(M, N, 3 * kk, K.KPR[BF16], CUS).split("/")[0] == cid.split("-")[0] and kk % seg == 0 and kk // seg >= 2, cid


def test_tails_of_the_gemm_cases():
    for cid, (M, N, _rows) in K.GEMM_CASES.items():
        rows, cols = (int(v) for v in K.form_of(cid).split("/")[0].replace("ring", "128x128").split("+")[0].split("x"))
        assert M % rows == 5 and M > rows and N % cols != 0, cid
    for cid in ("256x256+128/reg", "256x256+128/dma"):              # 8192 tall rows, then 2053 rows of 128-row tiles with a tail of 5
        M, N, _ = K.GEMM_CASES[cid]
        assert (K.tall_rows(M, N, CUS), M - K.tall_rows(M, N, CUS)) == (8192, 2053)


@pytest.mark.parametrize("layer", K.LAYERS)
def test_persistent_image_counts(layer):
    for mode, tile in (("f32", "wide"), ("bf16", "tall"), ("bf16", "wide"), ("bf16x3", "tall"), ("bf16x3", "wide")):
        g = K.conv_cfg(layer, mode, tile)
        n = K.persistent_n(g, CUS)
        bound = 2 * CUS // g["n_tiles_n"]
        tiles = K.conv_tiles(g, n)
        assert tiles > 2 * bound and tiles % bound != 0 and n % K.P_IMAGES != 0 and (g["IMGS"] == 1 or n % g["IMGS"] != 0)
        assert n < 1100, n
        if g["IMGS"] > 1:
            assert K.SMALL_N % g["IMGS"] != 0
    assert K.conv_cfg(2, "bf16", "tall")["TILES_Y"] == 4 and K.conv_cfg(6, "bf16", "tall")["IMGS"] == 4
    assert 256 < K.persistent_n(K.conv_cfg(2, "bf16", "tall"), CUS) < 270 and 1024 < K.persistent_n(K.conv_cfg(6, "bf16x3", "tall"), CUS) < 1040


def test_conv1_image_count():
    n = K.conv1_persistent_n(CUS)
    assert n * 12 > CUS * 4 and n * (96 // K.C["conv1_rows"]) > CUS * K.C["conv1_waves"] and n < 200


@pytest.mark.parametrize("kind", ["grid", "sparse9"])
@pytest.mark.parametrize("layer", [3, 6])
def test_conv_builders_and_references(layer, kind):
    """One unpooled and one pooled layer (the others differ in size only): planted content, exactness assertion, operand layouts."""
    c = K.conv_case(layer, kind)
    for mode in (("bf16x3",) if kind == "sparse9" else ("f32", "bf16")):
        x, wp, y = K.conv_operands(c, mode)
        g = c["g"]
        ka, kw = (2, 3) if mode == "bf16x3" else (1, 1)
        assert tuple(x.shape) == (K.P_IMAGES, g["H"], g["W"], ka * g["cin"]) and tuple(wp.shape) == (g["cout"], 9, kw * g["cin"])
        assert y.shape[-1] == ka * g["cout"] and y.shape[1] == (g["H"] // 2 if g["pool"] else g["H"])
        if mode == "bf16x3":
            assert int((y[..., g["cout"]:] != 0).sum()) > 0               # the expected lo plane is not empty


def test_gemm_builders_and_references():
    a, w, b = K.gemm_operands(1, 133, 300, 72)
    y, y_abs = K.gemm_reference(a, w, b)
    K.assert_exact_arithmetic(y_abs)
    assert torch.equal(K.cast(y, F32).double(), y)
    for cid, (M, N, kk, seg) in K.X3_GEMM_CASES.items():
        c = K.x3_gemm_case(5, M, N, kk)
        K.assert_exact_arithmetic(c["y_abs"], 2.0 ** -18)
        assert K.seg_planes_a(c["a"], seg).shape == (M, 2 * kk) and K.seg_planes_w(c["w"], seg).shape == (N, 3 * kk)
        assert int((K.split_out(c["y"].clamp_min(0))[:, N:] != 0).sum()) > 0
    # the longest reductions of the GPU file
    c = K.x3_gemm_case(6, 8, 8, 4608)
    K.assert_exact_arithmetic(c["y_abs"], 2.0 ** -18)


def test_conv1_and_helper_references():
    c = K.conv1_case("grid")
    y, y_abs = K.conv1_reference(c["x"], c["w"], c["b"])
    K.assert_exact_arithmetic(y_abs)
    assert tuple(y.shape) == (K.P_IMAGES, 48, 32, 64) and int((K.split_out(y)[..., 64:] != 0).sum()) > 0
    x = torch.cat([K.special_f32(), torch.randn(44)]).view(2, 32)
    p = K.split_reference(x[:, :32], 8, 2)
    assert p.shape == (2, 64) and torch.equal(p.view(2, 4, 2, 8)[:, :, 0].reshape(2, 32), x.to(BF16))
    assert K.merge_reference(p, 8).shape == (2, 32)
    assert torch.equal(K.split_reference(x, 16, 3).view(2, 2, 3, 16)[:, :, 2], K.split_reference(x, 16, 3).view(2, 2, 3, 16)[:, :, 0])
