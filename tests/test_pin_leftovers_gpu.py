"""GPU tests of the six kernel families that only a norm-wise figure at one or two shapes held: rn_stem_kernel, rn_stem_wgrad,
linear_narrow_kernel<N>, linear_small_kernel / linear_small_wide_kernel, mla_col_sum / mla_col_sum_bf16, and mla_bn_stats /
mla_bn_stats_fused up to 64 channels. ONE KERNEL CALL PER CHECK -- through ops, or through _lib where a pitch, an offset or a guard
region is needed -- against float64 torch computed from the same stored operands; every output element is compared.

Two kinds of checks, as in tests/test_infer_kernels_gpu.py:
  exact    operands on the dyadic grid (multiples of 2^-3 in [-1, 1]); the case asserts sum|terms| / unit < 2^24 from its float64
           reference, so any summation order gives the float64 value in f32: torch.equal (bf16: its round-to-nearest-even);
  derived  |got - ref| <= P 2^-24 sum|terms| per element, plus half a bf16 ulp for a bf16 output; P is counted from the kernel's code
           in the docstring of the bound (tests/pin_leftover_cases.py). Sums taken in double: count 2^-53 sum|terms| and the one f32
           rounding of the result. Each such check prints its worst error / bound before asserting <= 1. No bound here is measured.

Shapes, operand builders, references, bounds and the constants READ FROM THE SOURCES live in tests/pin_leftover_cases.py; they
evaluate without a device (tests/test_pin_leftover_cases_cpu.py)."""

import ctypes
import importlib

import pytest
import torch

import pin_leftover_cases as P
from conftest import PKG
from infer_kernel_cases import BF16, F32, cast
from test_wide_head_gpu import strided, within

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
SENTINEL = -7.0                          # fills whatever a kernel must not write
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


def ptr(t):
    return vp(t.data_ptr()) if t is not None else None


def pitched(t, pad, fill=NAN):
    """The same values with `pad` elements of `fill` behind every row; the base stays where the allocator put it (16-byte aligned)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device="cuda")
    view = buf[:, :t.shape[1]]
    view.copy_(t)
    return view


def guarded_out(M, N, pad, offset):
    """An (M, N) view with pitch N + pad that starts `offset` floats into a buffer of sentinels, and the buffer."""
    ldo = N + pad
    flat = torch.full((offset + M * ldo + 4,), SENTINEL, device="cuda")
    return flat, flat[offset:offset + M * ldo].view(M, ldo)[:, :N]


def assert_guards(flat, M, N, pad, offset, what):
    body = flat[offset:offset + M * (N + pad)].view(M, N + pad)
    assert bool((body[:, N:] == SENTINEL).all()) and bool((flat[:offset] == SENTINEL).all()) and bool((flat[offset + M * (N + pad):] == SENTINEL).all()), \
        what + ": wrote outside its (M, N) block"


# ---------------------------------------------------------------------------------------- 1. rn_stem forward ----

@pytest.mark.parametrize("dtype", [F32, BF16], ids=P.name)
@pytest.mark.parametrize("conf", P.STEM_CONFS)
@pytest.mark.parametrize("n", P.STEM_NS)
def test_rn_stem_every_element_within_its_derived_bound(ops, n, conf, dtype):
    """mla_rn_stem on 1 and 3 DIFFERENT images (the image index blockIdx.x / 112 beyond 0 and 1), both channel configurations, f32 and
    bf16 output, raw and through scale / shift + ReLU, against float64 conv2d of the normalised channels with the kernel's own f32
    constants. Every element, the outputs at oy, ox in {0, 1, 110, 111} like any other: a tap outside the image contributes nothing,
    and the planted border values raise the bound of the outputs that see them only. P = 55 and the two epilogue roundings:
    pin_leftover_cases.stem_bound."""
    c = P.stem_case(conf, n)
    planes, w = c["planes"].cuda(), c["w"].cuda()
    for scale, shift, relu, tag in ((None, None, False, "raw"), (c["scale"], c["shift"], True, "scale shift relu")):
        got = ops.rn_stem(planes, conf == "single", w, dtype, None if scale is None else scale.cuda(), None if shift is None else shift.cuda(), relu=relu)
        assert got.dtype == dtype and tuple(got.shape) == (n, 112, 112, 64)
        ref, bound = P.stem_bound(c["acc"], c["terms"], scale, shift, relu, dtype)
        within(got, ref, bound, "rn_stem %s n %d %s %s" % (conf, n, P.name(dtype), tag))


# ------------------------------------------------------------------------------------------ 2. rn_stem_wgrad ----

@pytest.mark.parametrize("conf", P.STEM_CONFS)
@pytest.mark.parametrize("n", P.WGRAD_NS)
def test_rn_stem_wgrad_every_element_within_its_derived_bound(ops, n, conf):
    """mla_rn_stem_wgrad at 1, 10 and 19 images (1, 2 and 3 output rows per block), both configurations, f32 and bf16 dy holding the
    same bf16-rounded values, against float64 conv2d_weight of the normalised input: every dw element within
    P 2^-24 sum|terms|, P = 28 rows_per_block + 7 (pin_leftover_cases.wgrad_p), beside the norm-wise 1e-4 (f32) / 1e-2 (bf16) of
    test_stem_wgrad_with_several_rows_per_block. The bf16 kernel differs from the f32 one in how it LOADS dy and in nothing else, so
    on the same values the two results must have the same bits -- which holds the bf16 run to the f32 figure."""
    c = P.wgrad_case(conf, n)
    planes, top = c["planes"].cuda(), float(c["ref"].abs().max())
    got = {}
    for dtype in (F32, BF16):
        dw = torch.full((64, 3, 7, 7), 9.0, device="cuda")
        ops.rn_stem_wgrad(planes, conf == "single", c["dy"].to(dtype).cuda(), dw)
        what = "rn_stem_wgrad %s n %d %s" % (conf, n, P.name(dtype))
        within(dw, c["ref"], c["bound"], what)
        e = float((dw.double().cpu() - c["ref"]).abs().max()) / top
        print("%s: max error over max value %.3g" % (what, e))
        assert e <= (1e-4 if dtype == F32 else 1e-2)
        got[dtype] = dw
    assert torch.equal(got[F32], got[BF16]), "f32 and bf16 dy of the same values gave different bits"


# -------------------------------------------------------------------------------------- 3. mla_linear_narrow ----

def run_linear(L, fn, a, w, b, N, pad=0, offset=0):
    M, Kk = a.shape
    flat, out = guarded_out(M, N, pad, offset)
    L.check(fn(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(b), ptr(out), N + pad, M, N, Kk, L.stream_ptr()))
    return flat, out


def check_linear(L, fn, c, N, pad, offset, what, input_pads=(0, 0)):
    """With and without the bias: the (M, N) block equals the float64 value, everything around it keeps its sentinel."""
    a, w, b = (c[k].cuda() for k in ("a", "w", "b"))
    if input_pads != (0, 0):
        a, w = pitched(a, input_pads[0]), pitched(w, input_pads[1])
    M = a.shape[0]
    for bias, key in ((b, "y"), (None, "y_nobias")):
        flat, out = run_linear(L, fn, a, w, bias, N, pad, offset)
        assert torch.equal(out, cast(c[key], F32).to(out.device)), "%s bias %s: not the float64 value" % (what, bias is not None)
        assert_guards(flat, M, N, pad, offset, what)
    return out


@pytest.mark.parametrize("N", P.NARROW_NS)
def test_linear_narrow_is_exact(L, N):
    """Every instantiation linear_narrow_kernel<1..16>, K in {4, 8, 64, 68, 600} (one float4 piece: lane 0 works alone; two; one per
    lane; lane 0 takes a second trip alone; 150 pieces: ragged), M in {1, 17} (one 16-lane group; a second block with one row), with
    and without bias, dense and with lda = K + 4, ldw = K + 8 (NaN behind every row) and ldo = N + 3 (sentinels that must survive).
    A wrong acc[] index in the `l == n` select or a wrong weight row shows: every (row, column) has its own value."""
    fn = L.lib().mla_linear_narrow
    for Kk in P.NARROW_KS:
        for M in P.NARROW_MS:
            c = P.linear_case(M, N, Kk)
            what = "linear_narrow %d x %d x %d" % (M, N, Kk)
            check_linear(L, fn, c, N, 0, 0, what + " dense")
            check_linear(L, fn, c, N, 3, 0, what + " pitched", input_pads=(4, 8))


def test_linear_narrow_past_the_grid_cap_is_exact(L):
    """M = 2048 * 16 + 5 at N = 10, K = 600 (79 MB of input): the rows of the second grid-stride trip and the last, partial group of
    16 rows. Reference in float64 on the device."""
    M, N, Kk = P.NARROW_BIG
    c = P.linear_case(M, N, Kk, device="cuda")
    check_linear(L, L.lib().mla_linear_narrow, c, N, 0, 0, "linear_narrow %d x %d x %d" % (M, N, Kk))


def test_linear_narrow_row_alone_equals_the_row_in_its_batch(L):
    """Uniform data with all mantissa bits, 37 rows of 600 -> 10: a row computed alone has the bits it has inside the batch (first
    row, a row of the second block, the last row)."""
    gen = torch.Generator().manual_seed(77)
    a, w, b = (torch.rand(s, generator=gen).cuda() * 2 - 1 for s in ((37, 600), (10, 600), (10,)))
    fn = L.lib().mla_linear_narrow
    batch = run_linear(L, fn, a, w, b, 10)[1]
    for r in (0, 16, 36):
        alone = run_linear(L, fn, a[r:r + 1].contiguous(), w, b, 10)[1]
        assert torch.equal(alone[0], batch[r]), r


# --------------------------------------------------------------------------------------- 4. mla_linear_small ----

@pytest.mark.parametrize("cid", list(P.SMALL_CASES))
def test_linear_small_is_exact(L, cid):
    """mla_linear_small on either side of every term of its form switch (N % 4, N >= 64, K <= 64, N K 4 <= 48 KiB, ldo % 4, out
    16-byte aligned, M N >= 65536), past the wide kernel's 1024-block cap, and at tiny shapes; with and without bias, dense inputs and
    lda = K + 1, ldw = K + 3 with NaN behind every row, sentinels around and between the rows of out. The form a case enters is
    evaluated from the pointer it was given and must be the one its id names."""
    M, N, Kk, pad, offset, form = P.SMALL_CASES[cid]
    c = P.linear_case(M, N, Kk)
    fn = L.lib().mla_linear_small
    out = check_linear(L, fn, c, N, pad, offset, "linear_small " + cid)
    assert P.small_form(M, N, Kk, N + pad, out.data_ptr() % 16 // 4) == form, cid
    check_linear(L, fn, c, N, pad, offset, "linear_small " + cid + " pitched inputs", input_pads=(1, 3))


def test_linear_small_forms_agree_bit_for_bit(L):
    """Uniform data with all mantissa bits, 600 outputs of K = 10: the wide form (110 rows), the plain form on the first 109 rows and
    the plain form on all rows through ldo = 602 give the same bits (k ascending, one fma chain, in both kernels)."""
    gen = torch.Generator().manual_seed(78)
    a, w, b = (torch.rand(s, generator=gen).cuda() * 2 - 1 for s in ((110, 10), (600, 10), (600,)))
    fn = L.lib().mla_linear_small
    assert P.small_form(110, 600, 10, 600, 0) == "wide" and P.small_form(109, 600, 10, 600, 0) == P.small_form(110, 600, 10, 602, 0) == "plain"
    wide = run_linear(L, fn, a, w, b, 600)[1]
    assert wide.data_ptr() % 16 == 0
    assert torch.equal(run_linear(L, fn, a[:109], w, b, 600)[1], wide[:109])
    assert torch.equal(run_linear(L, fn, a, w, b, 600, pad=2)[1], wide)


# ----------------------------------------------------------------------- 5. mla_col_sum, mla_col_sum_bf16 ----

def check_col_sum(ops, rows, dtype):
    for cols in P.COLSUM_COLS:
        x, ref = P.colsum_case(rows, cols)
        for form in P.COLSUM_FORMS[dtype]:
            left, right = P.colsum_layout(form, cols)
            xv = x.to(dtype).cuda() if form == "dense" else strided(x.to(dtype), left, right, fill=NAN)
            assert xv.stride(0) == cols + left + right or rows == 1
            if dtype == F32:
                assert (cols % 4 == 0 and xv.stride(0) % 4 == 0 and xv.data_ptr() % 16 == 0) == P.colsum_vector_form(form, cols)
            guard = torch.full((cols + 2,), SENTINEL, device="cuda")
            ops.col_sum(xv, guard[1:1 + cols])
            what = "col_sum %s %d x %d %s" % (P.name(dtype), rows, cols, form)
            assert torch.equal(guard[1:1 + cols].cpu(), cast(ref, F32)), what
            assert float(guard[0]) == SENTINEL and float(guard[-1]) == SENTINEL, what


@pytest.mark.parametrize("rows", P.COLSUM_ROWS[F32])
def test_col_sum_f32_is_exact(ops, rows):
    """mla_col_sum: chunks = clamp(rows / 64, 1, 64) of ceil(rows / chunks) rows -- one row, 63 / 64 / 127 (one chunk), 129 (two, the
    second one short), 4096 / 4097 (64 chunks; 65-row chunks with a two-row last one), 5120 (the cap); columns across the 64-column
    tiles of the scalar kernel and the 256-column tiles of the vector kernel with tails (1, 10, 64, 65, 256, 260, 600, 601); dense
    (16-byte loads when cols % 4 == 0), a pitch that is no multiple of 4 floats, and a base one float past a 16-byte boundary, NaN
    behind and in front of every row. Dyadic values: the double sums are exact and one cast gives the f32 value."""
    check_col_sum(ops, rows, F32)


@pytest.mark.parametrize("rows", P.COLSUM_ROWS[BF16])
def test_col_sum_bf16_is_exact(ops, rows):
    """mla_col_sum_bf16: chunks = clamp(rows / 256, 1, 64) -- one row, 255 / 256 (one chunk), 513 (two chunks of 257, the second one
    short by a row), 16384 / 16385 (64 chunks; 257-row chunks with a 194-row last one); the same columns, dense and pitched."""
    check_col_sum(ops, rows, BF16)


# -------------------------------------------------- 6. mla_bn_stats / mla_bn_stats_fused, 1..64 channels ----

def run_stats(L, ops, xv, mode, period, rm, rv, momentum, fused, tracked=None):
    rows, cols = xv.shape
    ch = P.stats_channels(mode, period, cols)
    mean, var = torch.full((ch,), SENTINEL, device="cuda"), torch.full((ch,), SENTINEL, device="cuda")
    ws, lib = ops._workspace(xv.device), L.lib()
    if fused:
        sums = torch.empty(2 * ch, dtype=torch.float64, device="cuda")
        L.check(lib.mla_bn_stats_fused(ptr(xv), rows, cols, xv.stride(0), mode, period, ptr(ws), ptr(sums), ptr(mean), ptr(var), ptr(rm), ptr(rv),
                                       float(momentum), ptr(tracked), L.stream_ptr()))
    else:
        L.check(lib.mla_bn_stats(ptr(xv), rows, cols, xv.stride(0), mode, period, ptr(ws), ptr(mean), ptr(var), ptr(rm), ptr(rv), float(momentum),
                                 L.stream_ptr()))
    return mean, var


def check_stats(L, ops, rows, cols, mode, period, layouts):
    """Per layout: mla_bn_stats within the per-channel bounds of pin_leftover_cases.stats_reference (mean, biased variance, running
    mean and running unbiased variance at momentum 0.1), the constant channel exactly (0.375, 0), mla_bn_stats_fused bit-identical
    with num_batches_tracked + 1; dense also: momentum < 0 with the pointers given leaves the running statistics' bits alone."""
    x, rm0, rv0, const = P.stats_input(rows, cols, mode, period)
    ref = P.stats_reference(x, rm0, rv0, mode, period)
    xd = x.cuda()
    for left, right in layouts:
        xv = xd if (left, right) == (0, 0) else strided(xd, left, right, fill=NAN)
        what = "bn_stats mode %d period %d %d x %d (+%d +%d) " % (mode, period, rows, cols, left, right)
        rm, rv = rm0.cuda(), rv0.cuda()
        mean, var = run_stats(L, ops, xv, mode, period, rm, rv, P.MOMENTUM, fused=False)
        for got, k in ((mean, "mean"), (var, "var"), (rm, "run_mean"), (rv, "run_var")):
            within(got, ref[k], ref["b_" + k], what + k)
        if const is not None:
            assert float(mean[const]) == P.CONSTANT and float(var[const]) == 0.0, what + "constant channel"
        if ref["count"] == 1:
            assert not bool(var.any()), what + "one element per channel: the variance is 0, biased or not"
        rm2, rv2, trk = rm0.cuda(), rv0.cuda(), torch.tensor(4, dtype=torch.int64, device="cuda")
        mean2, var2 = run_stats(L, ops, xv, mode, period, rm2, rv2, P.MOMENTUM, fused=True, tracked=trk)
        assert int(trk) == 5, what + "num_batches_tracked"
        for a, b, k in ((mean, mean2, "mean"), (var, var2, "var"), (rm, rm2, "run_mean"), (rv, rv2, "run_var")):
            assert torch.equal(a, b), what + "fused form " + k
        if (left, right) == (0, 0):
            for fused in (False, True):
                rm3, rv3 = rm0.cuda(), rv0.cuda()
                mean3, var3 = run_stats(L, ops, xv, mode, period, rm3, rv3, -1.0, fused=fused)
                assert torch.equal(rm3.cpu(), rm0) and torch.equal(rv3.cpu(), rv0), what + "momentum < 0 changed the running statistics"
                assert torch.equal(mean3, mean) and torch.equal(var3, var)


@pytest.mark.parametrize("period", P.STATS_PERIODS)
def test_bn_stats_row_mode_matches_float64(L, ops, period):
    """Mode 0 (channel = row % period; sums_rows_kernel, then reduce_finish_kernel up to 16 channels, partial_reduce_kernel +
    stats_finish_kernel above): periods 1, 10, 16, 17 (the switch), 64 (the limit); 1, 3, 512 and 1025 groups of rows -- 1025 is past
    kStatBlocks, so a block owns three groups and the last 170 blocks own none; 1, 4, 600, 601 columns, dense, misaligned (one float
    in front, two behind: scalar loads) and, for 4 and 600 columns, pitched by 4 floats (16-byte loads across a pitch). 1 x 1 with
    one group is a single element per channel. The eight combinations above 32 MB are left out (pin_leftover_cases)."""
    for rows, cols in P.stats_mode0_cases(period):
        check_stats(L, ops, rows, cols, 0, period, P.stats_layouts(cols))


@pytest.mark.parametrize("cols", P.STATS_COLS1)
def test_bn_stats_column_mode_matches_float64(L, ops, cols):
    """Mode 1 up to 64 columns (channel = column; sums_cols_kernel: 256 / cols row groups per block): 1, 10, 16, 17, 64 columns; 1 row
    (a single element per channel), 63 and 65 (one block, two blocks), 64 * 512 + 1 (kStatBlocks blocks of 65 rows, the last seven
    without a row); dense and misaligned."""
    for rows in P.STATS_ROWS1:
        check_stats(L, ops, rows, cols, 1, 0, [(0, 0), (1, 2)])
