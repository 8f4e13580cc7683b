"""CPU side of tests/test_cnn_train_bf16_gpu.py: the constants read from the sources parse, the case table names every compiled wgrad
shape and every line of conv_generic, the image counts reach the branches they are meant for at 256 CUs, and every operand builder,
float64 reference and exactness / planted-case / tie-share assertion of the GPU file evaluates without a device."""

import pytest
import torch

import cnn_train_bf16_cases as T
import infer_kernel_cases as K
from infer_kernel_cases import BF16

CUS = T.CUS_ASSUMED


def test_constants_read_from_the_sources():
    assert T.SHAPES == [(64, 128, 48, 32), (128, 256, 24, 16), (256, 256, 24, 16), (256, 512, 12, 8), (512, 512, 12, 8)]
    assert T.C["tco128"] in (0, 1) and T.C["c1_max_wg"] > 0 and T.C["bias_grid8"] > 0
    assert [T.wgrad_tiles(s[0], s[1]) for s in T.SHAPES] == ([1, 4, 8, 16, 32] if T.C["tco128"] else [1, 4, 8, 16, 32])
    assert [T.wgrad_bands(s) for s in T.SHAPES] == [12, 3, 3, 1, 1]


def test_wgrad_case_table_at_256_cus():
    cases = T.wgrad_cases(CUS)
    assert {s for _, s, _ in cases} == set(T.SHAPES)                   # every shape of MLA_WGRAD_SHAPES
    by_id = {cid: (s, n) for cid, s, n in cases}
    assert len(by_id) == len(cases) == 13
    assert [by_id["%d-%d-splits+1" % s[:2]][1] for s in T.SHAPES] == [257, 65, 33, 17, 9]
    assert by_id["256-512-2splits+1"][1] == 33 and by_id["512-512-2splits+1"][1] == 17
    for cid, s, n in cases:
        splits = min(T.wgrad_splits(s, CUS), n)
        n_mine = [(n - k + splits - 1) // splits for k in range(splits)]
        assert sum(n_mine) == n
        if cid.endswith("-splits+1"):
            assert n_mine[0] == 2 and set(n_mine[1:]) == {1}
        if cid.endswith("-2splits+1"):
            assert n_mine[0] == 3 and T.wgrad_bands(s) == 1            # three items in a BANDS == 1 workgroup: both LDS images re-used
        # the exactness condition from the element-wise worst case (every |term| at its largest): |a| <= 1, |dz| <= 1
        assert n * s[2] * s[3] * 1.0 / 2.0 ** (-2 * T.wgrad_bits(n)) < 2 ** 24, cid
    assert by_id["256-256-n1"][1] < T.wgrad_splits((256, 256, 24, 16), CUS)


def test_wgrad_matmul_reference_equals_autograd():
    """On grid values both forms are exact, so they agree bit for bit; so does sum|terms|. Also the planted rows."""
    shape = (256, 512, 12, 8)
    a, dz, unit = T.wgrad_operands(shape, 5, CUS)
    assert bool((a[0, 0] == 1).all() and (a[0, 11] == 1).all() and (a[4, 0] == 1).all()) and not bool((a[1, 0] == 1).all())
    for t in (a, dz):
        assert torch.equal(t.to(BF16).float(), t)
    ref = T.wgrad_autograd(a, dz)
    assert torch.equal(T.wgrad_matmul(a, dz, chunk=2), ref) and bool(ref.any())
    terms = T.wgrad_matmul(a, dz, absolute=True)
    assert torch.equal(terms, T.wgrad_autograd(a.abs(), dz.abs()))
    T.assert_exact(terms, unit)
    a3, dz3, unit3 = T.wgrad_operands((64, 128, 48, 32), 3, CUS)        # the finer grid of the small cases, at the longest sum
    assert unit3 == 2.0 ** -8
    T.assert_exact(T.wgrad_matmul(a3, dz3, absolute=True), unit3)


@pytest.mark.parametrize("n", [1, 3])
def test_conv1_bwd_reference_and_planted_cases(n):
    """conv1_bwd_reference asserts the tie rule, the zero threshold and the four positions on its own routing."""
    x, w, b, d = T.conv1_bwd_operands(n)
    assert float(x.min()) == -1.0 and float(x.max()) == 3.0 and float(w.abs().max()) <= 0.5
    dw, db, dw_abs, db_abs = T.conv1_bwd_reference(x, w, b, d)
    T.assert_exact(dw_abs, 2.0 ** -5)
    T.assert_exact(db_abs, 2.0 ** -3)
    assert not bool(dw[T.CH_OFF].any()) and float(db[T.CH_OFF]) == 0.0 and float(db[T.CH_TIE]) == float(d[..., T.CH_TIE].double().sum())
    assert torch.equal(dw.float().double(), dw) and torch.equal(db.float().double(), db)


def test_conv1_bwd_image_count_passes_the_workgroup_cap():
    assert 65 * 48 > 4 * T.C["c1_max_wg"] >= 64 * 48 and max(T.CONV1_NS) == 65
    assert 65 * 48 * 32 * 3.0 * 1.0 / 2.0 ** -5 < 2 ** 24             # element-wise worst case of dW: one term per pooled pixel, |g x| <= 3


def test_pool_shapes_and_references():
    lanes = T.C["bias_grid8"] * 256
    n, H, W, Cc = T.POOL_SHAPES[2]
    assert lanes < n * (H // 2) * (W // 2) * Cc // 8 < 2 * lanes and n * H * W * Cc // 8 > 4 * lanes
    assert [s[3] // 8 for s in T.POOL_SHAPES[:2]] == [1, 2] and all(s[0] * s[1] * s[2] * s[3] // 8 < lanes for s in T.POOL_SHAPES[:2])
    for shape in T.POOL_SHAPES:
        assert lanes % (shape[3] // 8) == 0
    for shape in T.POOL_SHAPES[:2]:
        for pool in (True, False):
            a, d = T.pool_operands(shape, pool)
            assert torch.equal(a.to(BF16).float(), a) and torch.equal(d.to(BF16).float(), d)
            dz = T.pool_reference(a, d, pool)
            assert tuple(dz.shape) == shape and torch.equal(dz.float().to(BF16).double(), dz)
        codes, d = T.codes_operands(shape)
        assert int(codes.max()) == 4 and codes[0, 0, 0, :8].tolist() == [0, 1, 2, 3, 4, 3, 2, 1]
        dz = T.route_by_codes(codes, d)
        assert float(dz[0, 0, 0, 0]) == 1.0 and float(dz[0, 0, 1, 1]) == 0.875 and float(dz[0, 1, 0, 2]) == 0.75 and float(dz[0, 1, 1, 3]) == 0.625
        assert float(dz[0, :2, :2, 4].abs().sum()) == 0.0 and float(dz[0, 1, 1, 5]) == 0.375
        win = dz.reshape(shape[0], shape[1] // 2, 2, shape[2] // 2, 2, shape[3]).sum(dim=(2, 4))
        assert torch.equal(win, torch.where(codes < 4, d.double(), torch.zeros(())))


def test_generic_case_table_names_every_line_of_conv_generic():
    assert len(T.C["generic_lines"]) == 13 and set(T.C["generic_lines"]) == T.generic_table()
    for shape in T.PERSISTENT_DGRAD + T.WIDE_DGRAD:
        assert shape in T.DGRAD_SHAPES
    g = T.generic_cfg(128, 64, 48, 32, "tall")
    assert (g["WM"], g["NS"], g["BN"], g["TH"], g["TILES_Y"], g["n_tiles_n"], g["IMGS"]) == (4, 2, 64, 12, 4, 1, 1)
    for layer in K.LAYERS:                      # the restated geometry agrees with the one read from conv_layer's Cfg<> lines
        cin, cout, H, W = T.layer_shape(layer)
        for tile in ("tall", "wide"):
            ref, got = K.conv_cfg(layer, "bf16", tile), T.generic_cfg(cin, cout, H, W, tile)
            assert all(ref[k] == got[k] for k in ("IMGS", "TH", "BN", "TILES_Y", "n_tiles_n")), (layer, tile)
    for shape in T.PERSISTENT_DGRAD:
        g = T.generic_cfg(*shape, "tall")
        n = K.persistent_n(g, CUS)
        assert K.conv_tiles(g, n) > 2 * (2 * CUS // g["n_tiles_n"]) and n < 1100


@pytest.mark.parametrize("shape", [(512, 256, 12, 8), (128, 64, 48, 32)])
def test_dgrad_builder_and_reference(shape):
    c = T.dgrad_case(shape)
    assert tuple(c["y"].shape) == (K.P_IMAGES, shape[2], shape[3], shape[1]) and torch.equal(c["dz"].to(BF16).float(), c["dz"])
    assert int((K.cast(c["y"], BF16).double() != c["y"]).sum()) > 0     # the bf16 store does round


@pytest.mark.parametrize("layer", T.POOLED_LAYERS)
def test_window_code_references_and_tie_share(layer):
    """The narrow operands: every pre-activation a bf16 value, at least 1 % of the windows tie for the maximum, every code occurs, and
    some window's maximum is exactly 0 without all four values being negative (code 4 by `> 0`, not by sign)."""
    c = T.narrow_case(layer)
    prepool, pooled, codes, ties, top = T.train_reference(c["pre"])
    assert float(ties.double().mean()) >= 0.01, float(ties.double().mean())
    assert bool((top == 0).any()) and set(codes.unique().tolist()) == {0, 1, 2, 3, 4}
    assert torch.equal(prepool.double(), c["pre"].clamp_min(0)) and torch.equal(codes == 4, pooled == 0)
    tied_on = ties & (top > 0)
    assert bool(tied_on.any()) and int(codes[tied_on].max()) <= 2        # a tie never routes to the last position
    # routing by codes is what autograd does on the stored pre-pool activation
    d = K.dyadic(torch.Generator().manual_seed(layer), tuple(codes.shape))[:2]
    assert torch.equal(T.route_by_codes(codes[:2], d), T.pool_reference(prepool[:2].float(), d, True, planted=False))


def test_grid_case_gives_exact_prepool_reference():
    c = K.conv_case(3, "grid")
    assert torch.equal(K.cast(c["pre"].clamp_min(0), BF16), K.cast(c["y"], BF16))        # layer 3 is un-pooled: y = relu(pre)
    c = K.conv_case(6, "grid")
    prepool, pooled, codes, ties, top = T.train_reference(c["pre"])
    assert torch.equal(pooled, K.cast(c["y"], BF16)) and set(codes.unique().tolist()) == {0, 1, 2, 3, 4}
